// aomarl_pyr_host.h -- the host half of the pyramid sensor (aomarl_pyr.hip): the validation of the desc and of the
// arguments of set_modulation / measure, the batch plan and the launch count of a measure.  Plain C++ without a HIP call
// and without a global, so that it also compiles into a stand-alone host program (pyr_host_check.cpp) that runs it under
// the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "../../include/aomarl.h"

#define PYR_NMIN 64
#define PYR_NMAX 2048
#define PYR_MAX_PAIRS 1024
// bytes the planes of a batch of (environment, modulation point) pairs may occupy: the row pass's output (n lit rows)
// and the column pass's (Nfft rows) of every pair, well inside the 256 MB last-level cache, so that each pass finds
// the previous one's output there
#define PYR_BATCH_BYTES (96ll << 20)

static inline std::string pyr_fmt(const char *fmt, double a = 0, double b = 0, double c = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return std::string(buf);
}

// 0 when the desc can be used; otherwise 1 and `err` names the field
static inline int pyr_validate(const aomarl_pyr_desc *d, std::string &err) {
  if (!d) { err = "pyr_create: null desc"; return 1; }
  if (d->Nfft < PYR_NMIN || d->Nfft > PYR_NMAX || (d->Nfft & (d->Nfft - 1)))
    { err = pyr_fmt("pyr_create: Nfft = %.0f: the transform size must be a power of two in 64..2048", d->Nfft); return 1; }
  if (d->n < 2 || (d->n & 1) || d->n > d->Nfft)
    { err = pyr_fmt("pyr_create: n = %.0f with Nfft = %.0f: the pupil array must be even-sided and fit the grid", d->n, d->Nfft); return 1; }
  if (d->nrebin < 1 || d->Nfft % d->nrebin)
    { err = pyr_fmt("pyr_create: nrebin = %.0f does not divide Nfft = %.0f", d->nrebin, d->Nfft); return 1; }
  if (d->nenv < 1 || d->nenv > 65535)        // (one grid row per environment)
    { err = pyr_fmt("pyr_create: nenv = %.0f: 1..65535 environments", d->nenv); return 1; }
  if (d->npts_max < 1 || d->npts_max > PYR_MAX_PAIRS)
    { err = pyr_fmt("pyr_create: npts_max = %.0f: 1..%.0f modulation points", d->npts_max, PYR_MAX_PAIRS); return 1; }
  const long long nb = d->Nfft / d->nrebin;
  if (d->nvalid < 1 || 4LL * d->nvalid > nb * nb)
    { err = pyr_fmt("pyr_create: nvalid = %.0f: four blocks of them must fit the %.0f x %.0f image", d->nvalid, (double)nb, (double)nb); return 1; }
  if ((long long)d->nenv * nb * nb > 0x7fffffffLL || (long long)d->nenv * d->n * d->n > 0x7fffffffLL)
    { err = pyr_fmt("pyr_create: nenv = %.0f: the images or phases of all environments exceed 2^31 - 1 elements", d->nenv); return 1; }
  if (!(d->lambda_um > 0.f) || !isfinite(d->lambda_um)) { err = pyr_fmt("pyr_create: lambda_um = %g: positive and finite", d->lambda_um); return 1; }
  if (!(d->nphotons > 0.f) || !isfinite(d->nphotons)) { err = pyr_fmt("pyr_create: nphotons = %g: positive and finite", d->nphotons); return 1; }
  if (d->batch_kib < 0) { err = pyr_fmt("pyr_create: batch_kib = %.0f must not be negative", d->batch_kib); return 1; }
  if (!isfinite(d->noise)) { err = pyr_fmt("pyr_create: noise = %g is not finite", d->noise); return 1; }
  if (!isfinite(d->thresh)) { err = pyr_fmt("pyr_create: thresh = %g is not finite", d->thresh); return 1; }
  if (!d->mpupil || !d->halfxy || !d->submask || !d->validsubsx || !d->validsubsy || (d->pixel_filter && !d->sincar))
    { err = "pyr_create: null array in the desc"; return 1; }
  double lit = 0;
  for (long long i = 0; i < (long long)d->n * d->n; i++) lit += (double)d->mpupil[i] * d->mpupil[i];
  if (!(lit > 0.0) || !isfinite(lit)) { err = "pyr_create: mpupil has no lit pixel"; return 1; }
  for (long long i = 0; i < 4LL * d->nvalid; i++)
    if (d->validsubsx[i] < 0 || d->validsubsx[i] >= nb || d->validsubsy[i] < 0 || d->validsubsy[i] >= nb)
      { err = pyr_fmt("pyr_create: validsubs[%.0f] lies outside the %.0f x %.0f image", (double)i, (double)nb, (double)nb); return 1; }
  return 0;
}

// cx, cy, w [npts] as set_modulation takes them: finite, weights not negative with a positive sum.  *wsum: the sum.
static inline int pyr_validate_modulation(const float *cx, const float *cy, const float *w, int npts, int npts_max,
                                          float s_scale, double *wsum, std::string &err) {
  if (!cx || !cy || !w) { err = "pyr_set_modulation: null array"; return 1; }
  if (npts < 1 || npts > npts_max)
    { err = pyr_fmt("pyr_set_modulation: npts = %.0f: 1..%.0f (npts_max of the desc)", npts, npts_max); return 1; }
  if (!(s_scale > 0.f) || !isfinite(s_scale)) { err = pyr_fmt("pyr_set_modulation: s_scale = %g: positive and finite", s_scale); return 1; }
  double s = 0;
  for (int k = 0; k < npts; k++) {
    if (!isfinite(cx[k]) || !isfinite(cy[k])) { err = pyr_fmt("pyr_set_modulation: point %.0f is not finite", k); return 1; }
    if (!(w[k] >= 0.f) || !isfinite(w[k])) { err = pyr_fmt("pyr_set_modulation: weight %.0f = %g: finite and not negative", k, w[k]); return 1; }
    s += (double)w[k];
  }
  if (!(s > 0.0)) { err = "pyr_set_modulation: the weights sum to zero"; return 1; }
  *wsum = s;
  return 0;
}

static inline int pyr_validate_measure(int nenv, int env_begin, int env_count, int flags, int method, bool have_seeds,
                                       float noise, std::string &err) {
  if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > nenv)
    { err = pyr_fmt("pyr_measure: environments %.0f .. +%.0f of %.0f", env_begin, env_count, nenv); return 1; }
  if (method < 0 || method > 3) { err = pyr_fmt("pyr_measure: method = %.0f: 0..3", method); return 1; }
  if (flags & ~AOMARL_PYR_NOISE) { err = pyr_fmt("pyr_measure: unknown flags %.0f", flags); return 1; }
  if ((flags & AOMARL_PYR_NOISE) && noise >= 0.f && !have_seeds)
    { err = "pyr_measure: noise asked for without seeds and frame counters"; return 1; }
  return 0;
}

// How the (environment, point) pairs of a measure are cut into batches.  The planes of `cap` pairs fit PYR_BATCH_BYTES.
// Every batch holds whole environments with all their points (env_b of them) when one environment's points fit, and
// otherwise pts_b points of ONE environment, so that the pass that sums over the points owns every pixel it adds to.
struct PyrPlan {
  int cw = 0;                  // columns per workgroup of the column pass: CW lines of Nfft complex numbers <= 64 KB of LDS
  int cap = 0;                 // pairs the planes are allocated for
  long long t1_stride = 0, t2_stride = 0;      // float2 per pair: n x Nfft, Nfft x Nfft
  int filt_env = 0;            // environments per pass of the pixel filter (two Nfft^2 complex planes each)
};
static inline PyrPlan pyr_plan(int n, int N, int nenv, int npts_max, long long budget = PYR_BATCH_BYTES) {
  PyrPlan p;
  p.cw = N <= 1024 ? 8 : 4;
  p.t1_stride = (long long)n * N;
  p.t2_stride = (long long)N * N;
  const long long per_pair = (p.t1_stride + p.t2_stride) * 8;
  long long cap = budget / per_pair;
  const long long all = (long long)nenv * npts_max;
  cap = cap < 1 ? 1 : (cap > PYR_MAX_PAIRS ? PYR_MAX_PAIRS : cap);
  p.cap = (int)(cap > all ? all : cap);
  long long fe = budget / (2 * p.t2_stride * 8);
  p.filt_env = (int)(fe < 1 ? 1 : (fe > nenv ? nenv : fe));
  return p;
}
// batch shape for `npts` points
static inline void pyr_batch(const PyrPlan &p, int npts, int *env_b, int *pts_b) {
  if (npts <= p.cap) { *pts_b = npts; *env_b = p.cap / npts; }
  else { *pts_b = p.cap; *env_b = 1; }
}
// kernel launches of one measure (the test of "no launch depends on the data")
static inline long long pyr_launch_count(const PyrPlan &p, int env_count, int npts, bool pixel_filter) {
  int env_b, pts_b;
  pyr_batch(p, npts, &env_b, &pts_b);
  const long long env_batches = (env_count + env_b - 1) / env_b, pt_batches = (npts + pts_b - 1) / pts_b;
  long long n = 3 * env_batches * pt_batches;
  if (pixel_filter) n += 4 * ((env_count + p.filt_env - 1) / p.filt_env);
  return n + 2;      // binning + noise, slopes
}
