// aomarl_lgs_host.h -- the host half of the laser-guide-star sensor (aomarl_lgs.hip): the validation of the desc and of
// the arguments of set_kernels / trace / measure (every refusal by name), the kernel's table in the lag domain, and the
// launch plan of a measure.  Plain C++ without a HIP call and without a global, so that it also compiles into a
// stand-alone host program (lgs_host_check.cpp) that runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <complex>
#include <string>
#include <vector>
#include "../../include/aomarl.h"

#define LGS_THREADS 256
#define LGS_PD 16            // the sizes the kernel is built for: pdiam = 16 phase pixels on N = 64 (the production files)
#define LGS_N 64
#define LGS_PD_S 8           // ... and pdiam = 8 on N = 32 (a pupil of 8 pixels per sub-aperture)
#define LGS_N_S 32
#define LGS_NPIX_MAX 32      // binned pixels per axis the workgroup's LDS holds

static inline std::string lgs_fmt(const char *fmt, double a = 0, double b = 0, double c = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return std::string(buf);
}

// 0 when the desc can be used; otherwise 1 and `err` names the field
static inline int lgs_validate(const aomarl_lgs_desc *d, std::string &err) {
  if (!d) { err = "lgs_create: null desc"; return 1; }
  if (!((d->pdiam == LGS_PD && d->N == LGS_N) || (d->pdiam == LGS_PD_S && d->N == LGS_N_S)))
    { err = lgs_fmt("lgs_create: pdiam = %.0f with N = %.0f: the kernel is built for pdiam = 16 with N = 64 and pdiam = 8 with N = 32", d->pdiam, d->N); return 1; }
  if (d->npix < 1 || d->npix > LGS_NPIX_MAX || d->nrebin < 1 || (long long)d->npix * d->nrebin > d->N)
    { err = lgs_fmt("lgs_create: npix = %.0f, nrebin = %.0f: a window of 1..32 pixels that fits N = %.0f", d->npix, d->nrebin, d->N); return 1; }
  if (d->nenv < 1 || d->nenv > 65535)        // (one grid row per environment)
    { err = lgs_fmt("lgs_create: nenv = %.0f: 1..65535 environments", d->nenv); return 1; }
  if (d->n < d->pdiam || d->n > 32768) { err = lgs_fmt("lgs_create: n = %.0f: the pupil array must hold a sub-aperture", d->n); return 1; }
  if (d->nvalid < 1 || d->nvalid > 65535) { err = lgs_fmt("lgs_create: nvalid = %.0f: 1..65535 sub-apertures", d->nvalid); return 1; }
  if ((long long)d->nenv * d->nvalid * d->npix * d->npix > 0x7fffffffLL || (long long)d->nenv * d->n * d->n > 0x7fffffffLL)
    { err = lgs_fmt("lgs_create: nenv = %.0f: the cubes or phases of all environments exceed 2^31 - 1 elements", d->nenv); return 1; }
  if (!(d->lambda_um > 0.f) || !isfinite(d->lambda_um)) { err = lgs_fmt("lgs_create: lambda_um = %g: positive and finite", d->lambda_um); return 1; }
  if (!(d->nphotons > 0.f) || !isfinite(d->nphotons)) { err = lgs_fmt("lgs_create: nphotons = %g: positive and finite", d->nphotons); return 1; }
  if (!isfinite(d->noise)) { err = lgs_fmt("lgs_create: noise = %g is not finite", d->noise); return 1; }
  if (!isfinite(d->cog_offset) || !isfinite(d->cog_scale)) { err = "lgs_create: cog_offset / cog_scale is not finite"; return 1; }
  if (!d->mpupil || !d->halfxy || !d->flux || !d->sub_x0 || !d->sub_y0) { err = "lgs_create: null array in the desc"; return 1; }
  for (int k = 0; k < d->nvalid; k++) {
    if (d->sub_x0[k] < 0 || d->sub_y0[k] < 0 || d->sub_x0[k] + d->pdiam > d->n || d->sub_y0[k] + d->pdiam > d->n)
      { err = lgs_fmt("lgs_create: sub-aperture %.0f lies outside the %.0f x %.0f pupil array", k, d->n, d->n); return 1; }
    if (!(d->flux[k] >= 0.f) || !isfinite(d->flux[k])) { err = lgs_fmt("lgs_create: flux[%.0f] = %g: finite and not negative", k, d->flux[k]); return 1; }
  }
  return 0;
}

// K [nvalid][N][N] as set_kernels takes it
static inline int lgs_validate_kernels(const float *K, int nvalid, int N, std::string &err) {
  if (!K) { err = "lgs_set_kernels: null array"; return 1; }
  for (int k = 0; k < nvalid; k++) {
    double s = 0;
    const float *p = K + (size_t)k * N * N;
    for (int i = 0; i < N * N; i++) {
      if (!isfinite(p[i]) || p[i] < 0.f) { err = lgs_fmt("lgs_set_kernels: kernel %.0f, pixel %.0f = %g: finite and not negative", k, i, p[i]); return 1; }
      s += (double)p[i];
    }
    if (!(s > 0.0)) { err = lgs_fmt("lgs_set_kernels: kernel %.0f sums to zero", k); return 1; }
  }
  return 0;
}

// The table of one kernel in the lag domain: Kt[(sy + L) * PD + sx] = sum_j K[jy][jx] exp(+2 pi i (jy sy + jx sx) / N),
// |sy| <= L = PD - 1, 0 <= sx <= L, separable, in double.  out: (2 L + 1) * PD pairs (re, im).
static inline void lgs_kernel_table(const float *K, int PD, int N, float *out) {
  const int L = PD - 1;
  std::vector<std::complex<double>> tw((size_t)N), A((size_t)N * PD);
  for (int m = 0; m < N; m++) tw[m] = std::polar(1.0, 2.0 * M_PI * (double)m / (double)N);
  for (int jy = 0; jy < N; jy++)
    for (int sx = 0; sx < PD; sx++) {
      std::complex<double> a = 0;
      for (int jx = 0; jx < N; jx++) a += (double)K[(size_t)jy * N + jx] * tw[(jx * sx) & (N - 1)];
      A[(size_t)jy * PD + sx] = a;
    }
  for (int sy = -L; sy <= L; sy++)
    for (int sx = 0; sx < PD; sx++) {
      std::complex<double> a = 0;
      for (int jy = 0; jy < N; jy++) a += A[(size_t)jy * PD + sx] * tw[(jy * sy) & (N - 1)];
      out[2 * ((size_t)(sy + L) * PD + sx)] = (float)a.real();
      out[2 * ((size_t)(sy + L) * PD + sx) + 1] = (float)a.imag();
    }
}

// dm1[l] = delta_l - 1 = -alt_l / gsalt of the trace: the guide star above every layer, at or above the ground
static inline int lgs_validate_trace(const float *dm1, int nlayers, int ctx_layers, int max_layers, int nenv, int env_begin,
                                     int env_count, int flags, int known_flags, std::string &err) {
  if (!dm1) { err = "lgs_trace: null dm1"; return 1; }
  if (nlayers != ctx_layers || nlayers < 0 || nlayers > max_layers)
    { err = lgs_fmt("lgs_trace: %.0f values for %.0f layers", nlayers, ctx_layers); return 1; }
  for (int l = 0; l < nlayers; l++)
    if (!(dm1[l] > -1.f) || !(dm1[l] <= 0.f))
      { err = lgs_fmt("lgs_trace: dm1[%.0f] = %g: delta - 1 = -alt / gsalt must lie in (-1, 0] (the guide star above the layer)", l, dm1[l]); return 1; }
  if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > nenv)
    { err = lgs_fmt("lgs_trace: environments %.0f .. +%.0f of %.0f", env_begin, env_count, nenv); return 1; }
  if (flags & ~known_flags) { err = lgs_fmt("lgs_trace: unknown flags %.0f", flags); return 1; }
  return 0;
}

static inline int lgs_validate_measure(int nenv, int env_begin, int env_count, int flags, bool have_seeds, bool have_image,
                                       float noise, std::string &err) {
  if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > nenv)
    { err = lgs_fmt("lgs_measure: environments %.0f .. +%.0f of %.0f", env_begin, env_count, nenv); return 1; }
  if (flags & ~(AOMARL_LGS_NOISE | AOMARL_LGS_WRITE_CUBE)) { err = lgs_fmt("lgs_measure: unknown flags %.0f", flags); return 1; }
  if ((flags & AOMARL_LGS_NOISE) && noise >= 0.f && !have_seeds)
    { err = "lgs_measure: noise asked for without seeds and frame counters"; return 1; }
  if ((flags & AOMARL_LGS_WRITE_CUBE) && !have_image) { err = "lgs_measure: AOMARL_LGS_WRITE_CUBE without an image array"; return 1; }
  return 0;
}

// The launch of a measure: one workgroup per (sub-aperture, environment); a second, one-thread-per-environment launch
// advances the frame counters when noise was drawn.  Nothing depends on the data.
struct LgsPlan {
  unsigned grid_x = 0, grid_y = 0, threads = LGS_THREADS;
  int window = 0, indi = 0;          // the window of the unrolled binmap: HR pixels indi .. indi + window - 1 per axis
  int launches = 0;
};
static inline LgsPlan lgs_plan(int nvalid, int env_count, int npix, int nrebin, int N, bool noisy) {
  LgsPlan p;
  p.grid_x = (unsigned)nvalid;
  p.grid_y = (unsigned)env_count;
  p.window = npix * nrebin;
  p.indi = (N - p.window) / 2 + ((p.window % 2 != N % 2) ? 1 : 0);       // geom_init.py:731-758
  p.launches = noisy ? 2 : 1;
  return p;
}
