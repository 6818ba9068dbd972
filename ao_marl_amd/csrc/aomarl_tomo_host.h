// aomarl_tomo_host.h -- the host half of laser tomography (aomarl_tomo.hip): the validation of the arguments of
// aomarl_tomo_trace and aomarl_tomo_cov (every refusal by name), the per-(star, layer) table of the covariance, and the
// covariance's scalar text (tomo_cov_entry: one element, for host and device alike -- the kernel runs it per thread,
// tomo_host_check.cpp runs it on the CPU against a plain-loop restatement).  Plain C++ without a HIP call and without a
// global, so that it also compiles into a stand-alone host program under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/aomarl.h"
#include "aomarl_groot_fn.h"

#define TOMO_THREADS 256
#define TOMO_TILE 16                 // k_tomo_cov: a workgroup owns a 16 x 16 tile of the matrix, a thread one element
#define TOMO_MAX_LAYERS 8            // (AOMARL_MAX_LAYERS)
#define TOMO_ARCSEC2RAD (2.0 * M_PI / (360.0 * 3600.0))
#define TOMO_KAPPA (1e-6 * 206265.0)

static inline std::string tomo_fmt(const char *fmt, double a = 0, double b = 0, double c = 0, double d = 0) {
  char buf[320];
  snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  return std::string(buf);
}

// ---- the trace.  dims[l]: the side of screen l; n: the side of the sensor's grid.  The footprint of star k on layer l
// is the trace's coordinate at the grid's corners, evaluated as the kernel evaluates it (float, one fused multiply-add).
static inline int tomo_validate_trace(const aomarl_tomo_desc *d, const void *planes, int ctx_layers, const int *dims, int n,
                                      int nenv, int env_begin, int env_count, int flags, int known_flags, std::string &err) {
  if (!d) { err = "tomo_trace: null desc"; return 1; }
  if (!planes) { err = "tomo_trace: null planes"; return 1; }
  if (d->nstars < 1 || d->nstars > AOMARL_TOMO_MAX_STARS)
    { err = tomo_fmt("tomo_trace: %.0f stars: 1..%.0f", d->nstars, AOMARL_TOMO_MAX_STARS); return 1; }
  if (d->nlayers != ctx_layers || d->nlayers < 0 || d->nlayers > TOMO_MAX_LAYERS)
    { err = tomo_fmt("tomo_trace: offsets for %.0f layers, the context has %.0f", d->nlayers, ctx_layers); return 1; }
  if (!d->off || !d->dm1) { err = "tomo_trace: null off / dm1"; return 1; }
  if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > nenv)
    { err = tomo_fmt("tomo_trace: environments %.0f .. +%.0f of %.0f", env_begin, env_count, nenv); return 1; }
  if ((long long)nenv * d->nstars * n * n > 0x7fffffffLL)
    { err = tomo_fmt("tomo_trace: the planes of %.0f environments and %.0f stars exceed 2^31 - 1 elements", nenv, d->nstars); return 1; }
  if (flags & ~known_flags) { err = tomo_fmt("tomo_trace: unknown flags %.0f", flags); return 1; }
  const float c = 0.5f * (float)(n - 1);
  for (int k = 0; k < d->nstars; k++)
    for (int l = 0; l < d->nlayers; l++) {
      const float m = d->dm1[k * d->nlayers + l];
      const float *o = d->off + 2 * (k * d->nlayers + l);
      if (!isfinite(o[0]) || !isfinite(o[1]))
        { err = tomo_fmt("tomo_trace: off of star %.0f, layer %.0f is not finite", k, l); return 1; }
      if (!(m > -1.f) || !(m <= 0.f))
        { err = tomo_fmt("tomo_trace: dm1 of star %.0f, layer %.0f = %g: delta - 1 = -alt / gsalt must lie in (-1, 0]", k, l, m); return 1; }
      for (int ax = 0; ax < 2; ax++)
        for (int corner = 0; corner < 2; corner++) {
          const float x = corner ? (float)(n - 1) : 0.f;
          const float f = fmaf(m, x - c, x + o[ax]);
          if (!(f >= 0.f) || !(f <= (float)(dims[l] - 1)))
            { err = tomo_fmt("tomo_trace: the footprint of star %.0f leaves screen %.0f: coordinate %.2f outside [0, %.0f] (declare the field in the parameter file)", k, l, f, dims[l] - 1); return 1; }
        }
    }
  return 0;
}

// ---- the covariance
static inline int tomo_validate_cov(const aomarl_tomo_cov_desc *d, const void *out, std::string &err) {
  if (!d) { err = "tomo_cov: null desc"; return 1; }
  if (!out) { err = "tomo_cov: null out"; return 1; }
  if (d->k_row < 1 || d->k_row > AOMARL_TOMO_MAX_STARS || d->k_col < 1 || d->k_col > AOMARL_TOMO_MAX_STARS)
    { err = tomo_fmt("tomo_cov: %.0f row stars, %.0f column stars: 1..%.0f", d->k_row, d->k_col, AOMARL_TOMO_MAX_STARS); return 1; }
  if (d->nlayers < 1 || d->nlayers > TOMO_MAX_LAYERS) { err = tomo_fmt("tomo_cov: %.0f layers: 1..%.0f", d->nlayers, TOMO_MAX_LAYERS); return 1; }
  if (d->n_row < 1 || d->n_col < 1 || 2LL * d->n_row * d->k_row > 0x7fffffffLL || 2LL * d->n_col * d->k_col > 0x7fffffffLL)
    { err = tomo_fmt("tomo_cov: %.0f row points, %.0f column points: at least one, 2 n K below 2^31", d->n_row, d->n_col); return 1; }
  if (!(d->d > 0.0) || !isfinite(d->d)) { err = tomo_fmt("tomo_cov: d = %g m: positive and finite", d->d); return 1; }
  if (!d->row_px || !d->row_py || !d->col_px || !d->col_py || !d->row_stars || !d->col_stars || !d->layers)
    { err = "tomo_cov: null array in the desc"; return 1; }
  double top = 0;
  for (int l = 0; l < d->nlayers; l++) {
    const double *y = d->layers + 3 * l;
    if (!isfinite(y[0]) || y[0] < 0 || !(y[1] > 0) || !isfinite(y[1]) || !(y[2] > 0) || !isfinite(y[2]))
      { err = tomo_fmt("tomo_cov: layer %.0f (alt %g, r0 %g, L0 %g): alt finite and not negative, r0 and L0 positive and finite", l, y[0], y[1], y[2]); return 1; }
    top = y[0] > top ? y[0] : top;
  }
  for (int side = 0; side < 2; side++) {
    const double *s = side ? d->col_stars : d->row_stars;
    const int K = side ? d->k_col : d->k_row;
    for (int k = 0; k < K; k++) {
      if (!isfinite(s[3 * k]) || !isfinite(s[3 * k + 1]))
        { err = tomo_fmt("tomo_cov: %.0f star %.0f: direction is not finite", side, k); return 1; }
      if (!(s[3 * k + 2] > top))     // (infinity passes: a natural star)
        { err = tomo_fmt("tomo_cov: star %.0f: gsalt = %g m is not above the highest layer (%g m)", k, s[3 * k + 2], top); return 1; }
    }
    const double *px = side ? d->col_px : d->row_px, *py = side ? d->col_py : d->row_py;
    const int n = side ? d->n_col : d->n_row;
    for (int i = 0; i < n; i++)
      if (!isfinite(px[i]) || !isfinite(py[i])) { err = tomo_fmt("tomo_cov: point %.0f is not finite", i); return 1; }
  }
  return 0;
}

// per (star, layer): delta, the layer shift alt theta (metres); per layer: the weight and L0
struct TomoStarLayer { double delta, sx, sy; };
struct TomoLayer { double w, L0; };

static inline void tomo_cov_tables(const aomarl_tomo_cov_desc *d, std::vector<TomoStarLayer> &rows,
                                   std::vector<TomoStarLayer> &cols, std::vector<TomoLayer> &lay) {
  lay.resize(d->nlayers);
  for (int l = 0; l < d->nlayers; l++) {
    const double k = TOMO_KAPPA / d->d, u = 0.5 / (2.0 * M_PI);
    lay[l].w = k * k * pow(d->layers[3 * l + 1], -5.0 / 3.0) * (u * u);
    lay[l].L0 = d->layers[3 * l + 2];
  }
  for (int side = 0; side < 2; side++) {
    std::vector<TomoStarLayer> &t = side ? cols : rows;
    const double *s = side ? d->col_stars : d->row_stars;
    const int K = side ? d->k_col : d->k_row;
    t.resize((size_t)K * d->nlayers);
    for (int k = 0; k < K; k++)
      for (int l = 0; l < d->nlayers; l++) {
        const double alt = d->layers[3 * l];
        TomoStarLayer &e = t[(size_t)k * d->nlayers + l];
        e.delta = 1.0 - alt / s[3 * k + 2];
        e.sx = s[3 * k] * TOMO_ARCSEC2RAD * alt;
        e.sy = s[3 * k + 1] * TOMO_ARCSEC2RAD * alt;
      }
  }
}

// One element: row point (pxi, pyi) seen from the star whose layer table is ra[0 .. nlayers), slope axis ea (0: x, 1: y);
// column point, table rb, axis eb.  Layers outer, then the taps (+,+), (+,-), (-,+), (-,-).
GR_HD double tomo_cov_entry(double pxi, double pyi, const TomoStarLayer *ra, int ea, double pxj, double pyj,
                            const TomoStarLayer *rb, int eb, const TomoLayer *lay, int nlayers, double d) {
  double acc = 0.0;
  for (int l = 0; l < nlayers; l++) {
    const double ux = (ra[l].delta * pxi + ra[l].sx) - (rb[l].delta * pxj + rb[l].sx);
    const double uy = (ra[l].delta * pyi + ra[l].sy) - (rb[l].delta * pyj + rb[l].sy);
    const double ha = 0.5 * d * ra[l].delta, hb = 0.5 * d * rb[l].delta;
    const double hw = 0.5 * lay[l].w;
#if defined(__HIPCC__)
#pragma unroll 1          // (one copy of the structure function's text per layer loop, not four)
#endif
    for (int t = 0; t < 4; t++) {
      const double s1 = (t & 2) ? -1.0 : 1.0, s2 = (t & 1) ? -1.0 : 1.0;
      const double x = ux + (ea == 0 ? s1 * ha : 0.0) - (eb == 0 ? s2 * hb : 0.0);
      const double y = uy + (ea == 1 ? s1 * ha : 0.0) - (eb == 1 ? s2 * hb : 0.0);
      acc -= (s1 * s2) * (hw * gr_rodconan(sqrt(x * x + y * y), lay[l].L0));
    }
  }
  return acc;
}
