// aomarl_trace_dev.h -- the device functions the environment's kernels (aomarl_kernels.hip, aomarl_wfs.hip,
// aomarl_target.hip) share with the translation units that trace or finish a PSF on the context's description:
// aomarl_capi_dmreg.hip, aomarl_lgs.hip, aomarl_tomo.hip, aomarl_field.hip.  Each is the one text every caller compiles; a unit that switches floating-point contraction off
// includes this header in front of its pragma, so that these keep the default contraction wherever they are inlined.
#pragma once
#include "aomarl_dev.h"

// =============================================================================================
// deformable mirrors
// Stack-array shape: materialised per env (dim x dim).  Tip-tilt: NOT materialised -- the two
// commands are kept in the DM's 4-float slot of st->dm_shape and every consumer evaluates
// c0*f0[p] + c1*f1[p] from the static planes (L2/MALL-resident, shared by all environments).
// =============================================================================================
__device__ __forceinline__ float dm_value(const DevSys &sys, const DevState &st, int e, int k, int x,
                                          int y) {
  const DevDm &D = sys.dms[k];
  const float *slot = st.dm_shape + (long long)e * sys.shape_stride + D.shape_off;
  if (D.type == AOMARL_DM_PZT) return slot[y * D.dim + x];
  const float2 f = reinterpret_cast<const float2 *>(D.influ)[y * D.dim + x];
  return slot[0] * f.x + slot[1] * f.y;
}

// =============================================================================================
// raytrace into a phase buffer (generic, bilinear) -- unfused API path
// =============================================================================================
__device__ __forceinline__ float bilinear_ring(const float *in, int N, int ox, int oy, float fx,
                                               float fy) {
  int ix = (int)floorf(fx), iy = (int)floorf(fy);
  float wx = fx - (float)ix, wy = fy - (float)iy;
  if (ix < 0 || iy < 0 || ix >= N || iy >= N) return 0.f;
  int ix1 = ix + 1 < N ? ix + 1 : ix, iy1 = iy + 1 < N ? iy + 1 : iy;
  float v00 = in[ring_idx(ix, iy, ox, oy, N)], v01 = in[ring_idx(ix1, iy, ox, oy, N)];
  float v10 = in[ring_idx(ix, iy1, ox, oy, N)], v11 = in[ring_idx(ix1, iy1, ox, oy, N)];
  return (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
}

// the mirrors of environment e seen from pixel (x, y) of the sensor's (TARGET: the target's) grid, added to v in
// controller order: the mirror part of k_raytrace, shared with k_lgs_trace (aomarl_lgs.hip), whose layers alone differ
template <bool TARGET>
__device__ __forceinline__ float trace_dms(const DevSys &sys, const DevState &st, int e, int x, int y, float v) {
  for (int k = 0; k < sys.ndm; k++) {
    const DevDm &D = sys.dms[k];
    const float fx = (float)x + (TARGET ? D.txo : D.wxo), fy = (float)y + (TARGET ? D.tyo : D.wyo);
    const int ix = (int)floorf(fx), iy = (int)floorf(fy);
    if (ix >= 0 && iy >= 0 && ix < D.dim && iy < D.dim) {
      const float wx = fx - (float)ix, wy = fy - (float)iy;
      const int ix1 = ix + 1 < D.dim ? ix + 1 : ix, iy1 = iy + 1 < D.dim ? iy + 1 : iy;
      float v00 = dm_value(sys, st, e, k, ix, iy);
      if (wx == 0.f && wy == 0.f) {
        v += v00;
      } else {
        float v01 = dm_value(sys, st, e, k, ix1, iy), v10 = dm_value(sys, st, e, k, ix, iy1);
        float v11 = dm_value(sys, st, e, k, ix1, iy1);
        v += (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
      }
    }
  }
  return v;
}

// trace_dms<TARGET>'s values one by one: vals[k] is what mirror k adds at pixel (x, y); bit k of the result: it adds
// (the pixel lies on the mirror).  Expression for expression trace_dms's.  (k_tomo_trace, aomarl_tomo.hip; TARGET: the
// science field, aomarl_field.hip.)
template <bool TARGET = false>
__device__ __forceinline__ unsigned trace_dm_values(const DevSys &sys, const DevState &st, int e, int x, int y,
                                                    float (&vals)[AOMARL_MAX_DMS]) {
  unsigned has = 0;
#pragma unroll
  for (int k = 0; k < AOMARL_MAX_DMS; k++) {
    vals[k] = 0.f;
    if (k < sys.ndm) {
      const DevDm &D = sys.dms[k];
      const float fx = (float)x + (TARGET ? D.txo : D.wxo), fy = (float)y + (TARGET ? D.tyo : D.wyo);
      const int ix = (int)floorf(fx), iy = (int)floorf(fy);
      if (ix >= 0 && iy >= 0 && ix < D.dim && iy < D.dim) {
        const float wx = fx - (float)ix, wy = fy - (float)iy;
        const int ix1 = ix + 1 < D.dim ? ix + 1 : ix, iy1 = iy + 1 < D.dim ? iy + 1 : iy;
        float v00 = dm_value(sys, st, e, k, ix, iy);
        if (wx == 0.f && wy == 0.f) {
          vals[k] = v00;
        } else {
          float v01 = dm_value(sys, st, e, k, ix1, iy), v10 = dm_value(sys, st, e, k, ix, iy1);
          float v11 = dm_value(sys, st, e, k, ix1, iy1);
          vals[k] = (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
        }
        has |= 1u << k;
      }
    }
  }
  return has;
}

// Target.comp_strehl(do_fit = True), the default of every get_strehl call in the reference
// (shesha/supervisor/components/targetCompass.py:139-159): the PSF peak fitted by two 1-D sincs, along x and along y
// through the maximum and its two neighbours: y(x) = A sinc(w (x - x0)); gain of one axis = A / y(0) = 1 / sinc(w x0).
// COMPASS's kernel is not in the reference tree: restated from its name and docstring (UNPINNED); the same
// algorithm as oracle/aoref.c:aoref_sinc_gain (Newton from the parabola through the three points, fall-backs).
__device__ __forceinline__ float sincf_(float t) { return fabsf(t) < 1e-2f ? 1.f - t * t * (1.f / 6.f) * (1.f - t * t * 0.05f) : __sinf(t) / t; }
__device__ __forceinline__ float dsincf_(float t) {
  return fabsf(t) < 1e-2f ? -t * (1.f / 3.f) * (1.f - t * t * 0.1f) : (__cosf(t) - __sinf(t) / t) / t;
}
__device__ inline float sinc_gain(float ym, float y0, float yp) {
  if (!(y0 > 0.f)) return 1.f;
  const float rm = ym / y0, rp = yp / y0;
  const float a = 0.5f * (rm + rp) - 1.f, b = 0.5f * (rp - rm);
  if (!(a < -1e-6f)) return 1.f;
  float x0 = fminf(0.5f, fmaxf(-0.5f, -b / (2.f * a)));
  const float gpar = 1.f - b * b / (4.f * a);
  float w = fminf(3.f, fmaxf(1e-3f, sqrtf(-6.f * a / gpar)));
  for (int it = 0; it < 8; it++) {
    const float f0 = sincf_(w * x0), d0 = dsincf_(w * x0);
    const float fm = sincf_(w * (1.f + x0)), dm = dsincf_(w * (1.f + x0));
    const float fp = sincf_(w * (1.f - x0)), dp = dsincf_(w * (1.f - x0));
    const float F1 = fm - rm * f0, F2 = fp - rp * f0;
    const float J11 = (1.f + x0) * dm - rm * x0 * d0, J12 = w * dm - rm * w * d0;
    const float J21 = (1.f - x0) * dp - rp * x0 * d0, J22 = -w * dp - rp * w * d0;
    const float det = J11 * J22 - J12 * J21;
    if (!(fabsf(det) > 1e-12f)) break;
    const float dw = (F1 * J22 - F2 * J12) / det, dx = (J11 * F2 - J21 * F1) / det;
    w = fminf(3.f, fmaxf(1e-3f, w - dw));
    x0 = fminf(0.6f, fmaxf(-0.6f, x0 - dx));
    if (fabsf(dw) + fabsf(dx) < 1e-6f) break;          // (quadratic convergence: 2 - 4 iterations)
  }
  const float g = 1.f / sincf_(w * x0);
  if (g >= 1.f && g < 1.5f) return g;
  return (gpar >= 1.f && gpar < 1.5f) ? gpar : 1.f;
}
// one axis (0: x, 1: y) of the fit of a W x W window whose maximum sits at `arg` (1 on the border: no fit)
__device__ inline float fit_axis_gain(const float *img, int W, int arg, int axis) {
  const int ay = arg / W, ax = arg - ay * W;
  if (ax == 0 || ay == 0 || ax == W - 1 || ay == W - 1) return 1.f;
  const int d = axis ? W : 1;
  return sinc_gain(img[arg - d], img[arg], img[arg + d]);
}

// The short-exposure window's fit, done where the window is formed (the PSF finish kernels run on the library's side
// stream, off the control chain): gain of both axes -> pend[W * W + 1].  One wave: argmax (lowest index on ties,
// like the commit's reduction and the oracle's scan), then lanes 0 / 1 solve the two axes.  Call behind a barrier that
// makes pend[0 .. W*W) visible.
__device__ __forceinline__ void psf_window_fit(float *pend, int W) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  float m = -1.f;
  int arg = 0;
  for (int o = lane; o < W * W; o += 64) { const float v = pend[o]; if (v > m) { m = v; arg = o; } }
  for (int d = 32; d >= 1; d >>= 1) {
    const float m2 = __shfl_xor(m, d);
    const int a2 = __shfl_xor(arg, d);
    if (m2 > m || (m2 == m && a2 < arg)) { m = m2; arg = a2; }
  }
  const float g = lane < 2 ? fit_axis_gain(pend, W, arg, lane) : 1.f;
  const float g1 = __shfl(g, 1);
  if (lane == 0) pend[W * W + 1] = g * g1;
}

// publish the pending PSF: LE accumulation, Strehl SE / LE, variance bookkeeping
__device__ __forceinline__ void strehl_commit_body(const DevSys &sys, const DevState &st, int env_begin, int blk,
                                                   const float *__restrict__ PEND) {
  __shared__ float r0[256], r1[256];
  __shared__ int ri[256], rl[256];
  const int W = 2 * sys.hw;
  const int e = env_begin + blk;
  const float *pend = PEND + (long long)blk * (W * W + 4);
  float *le = st.le_img + (long long)e * W * W;
  float mse = 0.f, mle = 0.f;
  int arg = 0, argl = 0;
  // (the first 256 threads of the block do the work: blocks of 256 -- every caller but k_small_actor_head -- all of them)
  const int nthr = min((int)blockDim.x, 256);
  if ((int)threadIdx.x < nthr) {
    for (int o = threadIdx.x; o < W * W; o += nthr) {
      const float p = pend[o];
      const float l = le[o] + p;
      le[o] = l;
      if (p > mse) { mse = p; arg = o; }
      if (l > mle) { mle = l; argl = o; }
    }
    r0[threadIdx.x] = mse; r1[threadIdx.x] = mle; ri[threadIdx.x] = arg; rl[threadIdx.x] = argl;
  }
  __syncthreads();
  // (ties go to the lower index, like the scans of the oracle: the sinc fit reads the neighbours of THAT pixel)
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) {
      const int t = threadIdx.x, u = t + o;
      if (r0[u] > r0[t] || (r0[u] == r0[t] && ri[u] < ri[t])) { r0[t] = r0[u]; ri[t] = ri[u]; }
      if (r1[u] > r1[t] || (r1[u] == r1[t] && rl[u] < rl[t])) { r1[t] = r1[u]; rl[t] = rl[u]; }
    }
    __syncthreads();
  }
  // comp_strehl(do_fit = True): the short exposure's fitted gain comes with the window (psf_window_fit, computed
  // where the window was formed: this kernel sits on the control chain's critical path); the long exposure's is
  // solved when somebody reads it (k_strehl_fit_le): slot 7 holds the un-fitted value until then.
  if (threadIdx.x == 0) {
    float *s = st.strehl + (long long)e * 8;
    const float cnt = s[4] + 1.f;
    const float var = pend[W * W];
    const int ay = ri[0] / W, ax = ri[0] - ay * W;
    s[0] = r0[0] / sys.ref_peak;
    s[1] = r1[0] / cnt / sys.ref_peak;
    s[2] = var;
    s[3] = s[3] + var;
    s[4] = cnt;
    s[5] = (ay == 0 || ax == 0 || ay == W - 1 || ax == W - 1) ? 1.f : 0.f;
    s[6] = r0[0] * pend[W * W + 1] / sys.ref_peak;
    s[7] = r1[0] / cnt / sys.ref_peak;
  }
}
