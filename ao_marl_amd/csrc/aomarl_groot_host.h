// aomarl_groot_host.h -- the host half of aomarl_groot_* (aomarl_groot.hip): validation of the descs and the tap lists
// of the three covariance models.  Plain C++ without a HIP call, so that it also compiles into a stand-alone host
// program (groot_host_check.cpp) that runs it under the address and undefined-behaviour sanitizers.
//
// Every model is  out[i][j] = sum_t w_t F_kind(t)(|p_j - p_i + o_t|; x0_t, L0_t)  over a tap list:
//   Cerr    (groot.py:145-186) per layer  1/2 w [D(r - s) + D(r + s) - 2 D(r)], D = dphi_lowpass: the reference's
//           Caniso + Cbp + Ccov telescope to D(r - s) - D(r), and adding the transpose turns -s into +s.  3 taps.
//   Calias  (:590-599, :633-700) the double loop over (k, p) only sees k - p: 2 npts - 1 offsets m h with the weights
//           sum(coeff[|m|:] coeff[:npts - |m|]) (:511-514), three taps each (-d, +d, twice the middle), dphi_highpass
//   dCmm    (:842-903) per layer 1/4 w ([R(r + d - v) + R(r - d - v) - 2 R(r - v)] - [the same with + v]), R = rodconan.
//           6 taps.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/aomarl.h"
#include "aomarl_groot_fn.h"

#define GR_MAX_LAYERS 64
#define GR_MAX_NPTS 33          // Simpson points of Calias
#define GR_MAX_BATCH 4096
#define GR_MAX_POINTS 16384

struct GrTap {
  double w, ox, oy, x0, L0;
  int32_t kind, pad;
};

static inline std::string gr_fmt(const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return std::string(buf);
}

static inline int gr_validate_create(const aomarl_groot_desc *d, std::string &err) {
  if (!d) { err = "groot_create: null desc"; return 1; }
  if (d->n_max < 1 || d->n_max > GR_MAX_POINTS)
    { err = gr_fmt("groot_create: n_max = %lld points (1..%lld)", d->n_max, GR_MAX_POINTS); return 1; }
  if (d->batch_max < 1 || d->batch_max > GR_MAX_BATCH)
    { err = gr_fmt("groot_create: batch_max = %lld (1..%lld)", d->batch_max, GR_MAX_BATCH); return 1; }
  if (d->m_max < 0 || d->m_max > GR_MAX_POINTS || d->k_max < 0 || d->k_max > 2 * GR_MAX_POINTS || (d->m_max > 0) != (d->k_max > 0))
    { err = gr_fmt("groot_create: m_max = %lld, k_max = %lld: the sandwich's sizes (both 0: no sandwich)", d->m_max, d->k_max);
      return 1; }
  if (!d->tabx || !d->taby) { err = "groot_create: null tabx / taby"; return 1; }
  for (int j = 0; j < GR_NTAB; j++) {
    if (!(d->tabx[j] > 0.0) || (j > 0 && !(d->tabx[j] > d->tabx[j - 1])))
      { err = gr_fmt("groot_create: tabx[%lld] does not ascend from a positive value", j); return 1; }
    if (!(d->taby[j] == d->taby[j]))
      { err = gr_fmt("groot_create: taby[%lld] is not a number", j); return 1; }
  }
  return 0;
}

// the weights of the 2 npts - 1 offsets of Calias: w[npts - 1 + m] for m = -(npts - 1) .. npts - 1
static inline int gr_simpson_offsets(int npts, std::vector<double> &w, std::string &err) {
  if (npts < 1 || npts > GR_MAX_NPTS || npts % 2 == 0)
    { err = gr_fmt("groot_form: npts = %lld: the Simpson rule takes an odd number of points (1..%lld)", npts, GR_MAX_NPTS);
      return 1; }
  std::vector<double> c((size_t)npts, 1.0);
  for (int i = 1; i < npts; i += 2) c[i] = 4.0;
  for (int i = 2; i < npts - 1; i += 2) c[i] = 2.0;
  w.assign((size_t)(2 * npts - 1), 0.0);
  for (int m = 0; m < npts; m++) {
    double s = 0.0;
    for (int k = m; k < npts; k++) s += c[k] * c[k - m];
    w[npts - 1 + m] = w[npts - 1 - m] = s;
  }
  return 0;
}

static inline int gr_taps_per_entry(const aomarl_groot_form_desc *f) {
  if (f->model == AOMARL_GROOT_CERR) return 3 * f->nlayers;
  if (f->model == AOMARL_GROOT_CALIAS_XX || f->model == AOMARL_GROOT_CALIAS_YY) return 3 * (2 * f->npts - 1);
  return 6 * f->nlayers;
}

// 0 when the call can be made; otherwise 1 and `err` names the argument
static inline int gr_validate_form(const aomarl_groot_form_desc *f, int n, int ldo, long long stride_o, int n_max,
                                   int batch_max, std::string &err) {
  if (!f) { err = "groot_form: null desc"; return 1; }
  if (f->model < AOMARL_GROOT_CERR || f->model > AOMARL_GROOT_DCMM_YY)
    { err = gr_fmt("groot_form: model = %lld is none of the five", f->model); return 1; }
  const bool alias = f->model == AOMARL_GROOT_CALIAS_XX || f->model == AOMARL_GROOT_CALIAS_YY;
  if (f->batch < 1 || f->batch > batch_max)
    { err = gr_fmt("groot_form: batch = %lld, the object was created for 1..%lld", f->batch, batch_max); return 1; }
  if (n < 1 || n > n_max) { err = gr_fmt("groot_form: n = %lld points, the object was created for 1..%lld", n, n_max); return 1; }
  if (ldo < n || (f->batch > 1 && stride_o < (long long)(n - 1) * ldo + n))
    { err = gr_fmt("groot_form: ldo = %lld, stride_o = %lld do not hold %lld columns per row", ldo, stride_o, n); return 1; }
  if (alias) {
    std::vector<double> w;
    if (gr_simpson_offsets(f->npts, w, err)) return 1;
    if (f->nlayers != 1) { err = gr_fmt("groot_form: nlayers = %lld: the aliasing model has one weight per entry", f->nlayers); return 1; }
  } else if (f->nlayers < 1 || f->nlayers > GR_MAX_LAYERS)
    { err = gr_fmt("groot_form: nlayers = %lld (1..%lld)", f->nlayers, GR_MAX_LAYERS); return 1; }
  if (!(f->x0 > 0.0)) { err = "groot_form: x0 must be positive (actuator pitch or sub-aperture size)"; return 1; }
  if (!f->w) { err = "groot_form: null w"; return 1; }
  if (!alias && (!f->sx || !f->sy || !f->L0)) { err = "groot_form: null sx / sy / L0"; return 1; }
  for (long long i = 0; i < (long long)f->batch * f->nlayers; i++) {
    if (!std::isfinite(f->w[i])) { err = gr_fmt("groot_form: w[%lld] is not finite", i); return 1; }
    if (alias) continue;
    if (!std::isfinite(f->sx[i]) || !std::isfinite(f->sy[i])) { err = gr_fmt("groot_form: sx / sy[%lld] is not finite", i); return 1; }
    if (!(f->L0[i] > 0.0) || !std::isfinite(f->L0[i])) { err = gr_fmt("groot_form: L0[%lld] must be positive and finite", i); return 1; }
  }
  if (!std::isfinite(f->x0)) { err = "groot_form: x0 must be positive (actuator pitch or sub-aperture size) and finite"; return 1; }
  return 0;
}

static inline GrTap gr_tap(double w, double ox, double oy, double x0, double L0, int kind) {
  GrTap t;
  t.w = w; t.ox = ox; t.oy = oy; t.x0 = x0; t.L0 = L0; t.kind = kind; t.pad = 0;
  return t;
}

// taps [batch][gr_taps_per_entry], in the order the kernel sums them.  Call after gr_validate_form.
static inline void gr_build_taps(const aomarl_groot_form_desc *f, std::vector<GrTap> &taps) {
  taps.clear();
  const double d = f->x0;
  for (int b = 0; b < f->batch; b++) {
    if (f->model == AOMARL_GROOT_CERR) {
      for (int l = 0; l < f->nlayers; l++) {
        const size_t k = (size_t)b * f->nlayers + l;
        const double w = f->w[k], sx = f->sx[k], sy = f->sy[k], L0 = f->L0[k];
        taps.push_back(gr_tap(0.5 * w, -sx, -sy, d, L0, GR_KIND_LOWPASS));
        taps.push_back(gr_tap(0.5 * w, sx, sy, d, L0, GR_KIND_LOWPASS));
        taps.push_back(gr_tap(-w, 0.0, 0.0, d, L0, GR_KIND_LOWPASS));
      }
    } else if (f->model == AOMARL_GROOT_CALIAS_XX || f->model == AOMARL_GROOT_CALIAS_YY) {
      std::vector<double> wm;
      std::string err;
      gr_simpson_offsets(f->npts, wm, err);
      const double h = f->npts > 1 ? d / (f->npts - 1) : 1.0, w = f->w[b];
      const bool xx = f->model == AOMARL_GROOT_CALIAS_XX;
      for (int m = -(f->npts - 1); m <= f->npts - 1; m++) {
        const double wk = w * wm[(size_t)(f->npts - 1 + m)], o = m * h;
        taps.push_back(xx ? gr_tap(wk, -d, o, d, 1.0, GR_KIND_HIGHPASS) : gr_tap(wk, o, -d, d, 1.0, GR_KIND_HIGHPASS));
        taps.push_back(xx ? gr_tap(wk, d, o, d, 1.0, GR_KIND_HIGHPASS) : gr_tap(wk, o, d, d, 1.0, GR_KIND_HIGHPASS));
        taps.push_back(xx ? gr_tap(-2.0 * wk, 0.0, o, d, 1.0, GR_KIND_HIGHPASS) : gr_tap(-2.0 * wk, o, 0.0, d, 1.0, GR_KIND_HIGHPASS));
      }
    } else {
      const bool xx = f->model == AOMARL_GROOT_DCMM_XX;
      const double dx = xx ? d : 0.0, dy = xx ? 0.0 : d;
      for (int l = 0; l < f->nlayers; l++) {
        const size_t k = (size_t)b * f->nlayers + l;
        const double w = 0.25 * f->w[k], vx = f->sx[k], vy = f->sy[k], L0 = f->L0[k];
        taps.push_back(gr_tap(w, dx - vx, dy - vy, d, L0, GR_KIND_RODCONAN));
        taps.push_back(gr_tap(w, -dx - vx, -dy - vy, d, L0, GR_KIND_RODCONAN));
        taps.push_back(gr_tap(-2.0 * w, -vx, -vy, d, L0, GR_KIND_RODCONAN));
        taps.push_back(gr_tap(-w, -dx + vx, -dy + vy, d, L0, GR_KIND_RODCONAN));
        taps.push_back(gr_tap(-w, dx + vx, dy + vy, d, L0, GR_KIND_RODCONAN));
        taps.push_back(gr_tap(2.0 * w, vx, vy, d, L0, GR_KIND_RODCONAN));
      }
    }
  }
}

static inline int gr_validate_sandwich(int m, int n, int ldg, int ldc, int ldo, const void *G, const void *C, const void *out,
                                       int m_max, int k_max, std::string &err) {
  if (m_max < 1) { err = "groot_sandwich: the object was created without a sandwich (m_max = 0)"; return 1; }
  if (m < 1 || m > m_max) { err = gr_fmt("groot_sandwich: m = %lld rows, the object was created for 1..%lld", m, m_max); return 1; }
  if (n < 1 || n > k_max) { err = gr_fmt("groot_sandwich: n = %lld, the object was created for 1..%lld", n, k_max); return 1; }
  if (!G || !C || !out) { err = "groot_sandwich: null operand"; return 1; }
  if (ldg < n || (ldg & 3) || ((uintptr_t)G & 15))
    { err = gr_fmt("groot_sandwich: ldg = %lld: G's rows must hold %lld columns, be a multiple of 4 floats long and 16-byte aligned",
                   ldg, n); return 1; }
  if (ldc < n || (ldc & 3) || ((uintptr_t)C & 15))
    { err = gr_fmt("groot_sandwich: ldc = %lld: C's rows must hold %lld columns, be a multiple of 4 floats long and 16-byte aligned",
                   ldc, n); return 1; }
  if (ldo < m) { err = gr_fmt("groot_sandwich: ldo = %lld for %lld columns", ldo, m); return 1; }
  return 0;
}
