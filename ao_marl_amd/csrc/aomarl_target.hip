// aomarl_target.hip -- the science-target stage of the environment: the windowed PSF as a separable DFT (k_target_rows,
// k_target_rows_mfma, k_target_rows_fast; k_target_finish, k_target_finish_mfma), the Strehl record (k_strehl_commit,
// k_strehl_fit_le, k_strehl_reset), and their launchers: a translation unit of its own.  It sees the device description
// (aomarl_dev.h) and a plan (aomarl_stage_plan_host.h) through aomarl_stage_host.h, not the context.  The dynamic LDS a
// rows kernel carves up is sized by plan_target from the constants the kernel itself uses (TGT_*).
#include "aomarl_stage_host.h"
#include "aomarl_trace_dev.h"
#include "aomarl_spot_dev.h"          // add4, add4_ring, mfma16: shared with aomarl_frame.hip

// =============================================================================================
// science target: fused raytrace + windowed PSF (separable DFT) + phase variance
// stage 1: R[y][kx] = sum_x a(y, x) exp(-2 pi i kx x / Npsf), kx in [-hw, hw)
// =============================================================================================
// (TGT_XC, TGT_TILE, TGT_TILE_PITCH, TGT_RED_*, TGT_TW_MAX: aomarl_stage_plan_host.h, where plan_target sizes the LDS from them)
template <bool FROM_BUF>
__global__ __launch_bounds__(256) void k_target_rows(DevSys sys, DevState st, int env_begin,
                                                     float *__restrict__ TR,
                                                     float *__restrict__ TPART, int nblk) {
  extern __shared__ float smem[];
  const int W = 2 * sys.hw, RB = 256 / W, pd = sys.pupdiam, np = sys.npsf;
  float *sar = smem;                      // [RB][TGT_XC]
  float *sai = sar + RB * TGT_XC;
  float *red = sai + RB * TGT_XC;         // [3][256]
  float2 *stw = reinterpret_cast<float2 *>(red + TGT_RED_VALU);   // [np] (only if it fits)
  const bool tw_lds = np <= TGT_TW_MAX;
  const int tid = threadIdx.x;
  const int e = env_begin + blockIdx.y;
  const int y0 = blockIdx.x * RB;
  const float2 *gtw = reinterpret_cast<const float2 *>(sys.psf_tw);
  if (tw_lds)
    for (int j = tid; j < np; j += 256) stw[j] = gtw[j];
  const float2 *tw = tw_lds ? stw : gtw;
  // pivot for the variance sums: phase at the pupil-grid centre
  float pivot;
  {
    const int cx = pd / 2, cy = pd / 2;
    float v = 0.f;
    if (FROM_BUF) {
      v = st.tar_phase[(long long)e * pd * pd + cy * pd + cx];
    } else {
      for (int l = 0; l < sys.nlayers; l++) {
        const DevLayer &L = sys.layers[l];
        const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
        const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
        v += base[ring_idx(cx + L.tox, cy + L.toy, ox, oy, L.dim)];
      }
      for (int k = 0; k < sys.ndm; k++)
        v += dm_value(sys, st, e, k, cx + sys.dms[k].tox, cy + sys.dms[k].toy);
    }
    pivot = v;
  }
  const int kxi = tid % W, ys = tid / W;
  const int kxf = kxi - sys.hw;
  float accr = 0.f, acci = 0.f;
  float sd = 0.f, sd2 = 0.f, sm = 0.f;
  for (int x0 = 0; x0 < pd; x0 += TGT_XC) {
    __syncthreads();
    for (int p = tid; p < RB * TGT_XC; p += 256) {
      const int yy = p / TGT_XC, xx = p - yy * TGT_XC;
      const int y = y0 + yy, x = x0 + xx;
      float ar = 0.f, ai = 0.f;
      if (y < pd && x < pd) {
        const float m = sys.spupil[y * pd + x];
        if (m != 0.f) {
          float v = 0.f;
          if (FROM_BUF) {
            v = st.tar_phase[(long long)e * pd * pd + y * pd + x];
          } else {
            for (int l = 0; l < sys.nlayers; l++) {
              const DevLayer &L = sys.layers[l];
              const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
              const int ox = st.origin[(e * sys.nlayers + l) * 2];
              const int oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
              v += base[ring_idx(x + L.tox, y + L.toy, ox, oy, L.dim)];
            }
            for (int k = 0; k < sys.ndm; k++)
              v += dm_value(sys, st, e, k, x + sys.dms[k].tox, y + sys.dms[k].toy);
          }
          float t = v * sys.tar_inv_lambda;
          t -= rintf(t);
          float sn, cs;
          sincospif(2.0f * t, &sn, &cs);
          ar = m * cs; ai = m * sn;
          const float d = v - pivot;
          sd += d; sd2 += d * d; sm += 1.f;
        }
      }
      sar[p] = ar; sai[p] = ai;
    }
    __syncthreads();
    if (ys < RB) {
      const int xmax = (pd - x0) < TGT_XC ? (pd - x0) : TGT_XC;
      for (int xx = 0; xx < xmax; xx++) {
        const float ar = sar[ys * TGT_XC + xx], ai = sai[ys * TGT_XC + xx];
        const float2 w = tw[(kxf * (x0 + xx)) & (np - 1)];   // (cos, sin); e^{-i t} = cos - i sin
        accr += ar * w.x + ai * w.y;
        acci += ai * w.x - ar * w.y;
      }
    }
  }
  if (ys < RB && y0 + ys < pd) {
    float *o = TR + (((long long)blockIdx.y * pd + (y0 + ys)) * W + kxi) * 2;
    o[0] = accr; o[1] = acci;
  }
  // block partial sums for the variance
  red[tid] = sd; red[256 + tid] = sd2; red[512 + tid] = sm;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; red[512 + tid] += red[512 + tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float *pp = TPART + ((long long)blockIdx.y * nblk + blockIdx.x) * 4;
    pp[0] = red[0]; pp[1] = red[256]; pp[2] = red[512]; pp[3] = 0.f;
  }
}

// (the sinc fit of the PSF peak -- sinc_gain, fit_axis_gain, psf_window_fit: aomarl_trace_dev.h)

// stage 2: G[ky][kx] = sum_y R[y][kx] exp(-2 pi i ky y / Npsf); |G|^2 -> pending window;
// variance from the block partials -> pending[W*W]
__global__ __launch_bounds__(256) void k_target_finish(DevSys sys, const float *__restrict__ TR,
                                                       const float *__restrict__ TPART, int nblk,
                                                       float *__restrict__ PEND) {
  const int W = 2 * sys.hw, pd = sys.pupdiam, np = sys.npsf;
  const int b = blockIdx.x;     // env within the batch
  const float2 *tw = reinterpret_cast<const float2 *>(sys.psf_tw);
  const float2 *R = reinterpret_cast<const float2 *>(TR) + (long long)b * pd * W;
  float *pend = PEND + (long long)b * (W * W + 4);
  for (int o = threadIdx.x; o < W * W; o += blockDim.x) {
    const int ky = o / W, kx = o - ky * W;
    const int kyf = ky - sys.hw;
    float gr = 0.f, gi = 0.f;
    for (int y = 0; y < pd; y++) {
      const float2 r = R[y * W + kx];
      const float2 w = tw[(kyf * y) & (np - 1)];
      gr += r.x * w.x + r.y * w.y;
      gi += r.y * w.x - r.x * w.y;
    }
    pend[o] = gr * gr + gi * gi;
  }
  __syncthreads();
  psf_window_fit(pend, W);
  if (threadIdx.x == 0) {
    double sd = 0., sd2 = 0., sm = 0.;
    for (int k = 0; k < nblk; k++) {
      const float *pp = TPART + ((long long)b * nblk + k) * 4;
      sd += pp[0]; sd2 += pp[1]; sm += pp[2];
    }
    double var = 0.;
    if (sm > 0.) { double mean = sd / sm; var = sd2 / sm - mean * mean; }
    pend[W * W] = (float)var;
  }
}


// ---------------------------------------------------------------------------------------------
// MFMA version (hw == 8 -> 16 kept frequencies per axis = one 16-wide MFMA tile).
// Block = 16 pupil rows; the complex amplitude of a 16 x 64 chunk is staged in LDS; the 4 waves
// split the chunk's 64 columns (K) and accumulate R[16 y][16 kx] with v_mfma_f32_16x16x4_f32:
//   Rr += ar*C + ai*S ; Ri += ai*C - ar*S ,  C/S[x][kx] = cos/sin(2 pi kx x / Npsf)
// ---------------------------------------------------------------------------------------------
template <bool FROM_BUF>
__global__ __launch_bounds__(256) void k_target_rows_mfma(DevSys sys, DevState st, int env_begin,
                                                          float *__restrict__ TR,
                                                          float *__restrict__ TPART, int nblk) {
  extern __shared__ float smem[];
  const int pd = sys.pupdiam, np = sys.npsf;
  float *sar = smem;                       // [16][65]
  float *sai = sar + TGT_TILE;
  float *red = sai + TGT_TILE;              // [4 waves][2][256] partial tiles; reused for sums
  float2 *stw = reinterpret_cast<float2 *>(red + TGT_RED_MFMA);   // [np] if it fits
  const bool tw_lds = np <= TGT_TW_MAX;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, c = lane & 15;
  const int e = env_begin + blockIdx.y;
  const int y0 = blockIdx.x * 16;
  const float2 *gtw = reinterpret_cast<const float2 *>(sys.psf_tw);
  if (tw_lds)
    for (int j = tid; j < np; j += 256) stw[j] = gtw[j];
  const float2 *tw = tw_lds ? stw : gtw;
  float pivot;
  {
    const int cx = pd / 2, cy = pd / 2;
    float v = 0.f;
    if (FROM_BUF) {
      v = st.tar_phase[(long long)e * pd * pd + cy * pd + cx];
    } else {
      for (int l = 0; l < sys.nlayers; l++) {
        const DevLayer &L = sys.layers[l];
        const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
        const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
        v += base[ring_idx(cx + L.tox, cy + L.toy, ox, oy, L.dim)];
      }
      for (int k = 0; k < sys.ndm; k++)
        v += dm_value(sys, st, e, k, cx + sys.dms[k].tox, cy + sys.dms[k].toy);
    }
    pivot = v;
  }
  f32x4 Rr = {0.f, 0.f, 0.f, 0.f}, Ri = {0.f, 0.f, 0.f, 0.f};
  float sd = 0.f, sd2 = 0.f, sm = 0.f;
  const int fy = tid >> 4, fx0 = (tid & 15) * 4;     // fill: row fy, 4 consecutive columns
  const int y = y0 + fy;
  const int kxf = c - 8;
  for (int x0 = 0; x0 < pd; x0 += 64) {
    __syncthreads();
    {
      float ph[4] = {0.f, 0.f, 0.f, 0.f};
      float mk[4] = {0.f, 0.f, 0.f, 0.f};
      const int xb = x0 + fx0;
      if (y < pd) {
        // pd % 4 == 0 (checked at create): a group of 4 columns is entirely inside or outside
        if (xb < pd) add4(mk, sys.spupil + y * pd + xb);
        if (FROM_BUF) {
          if (xb < pd) add4(ph, st.tar_phase + (long long)e * pd * pd + y * pd + xb);
        } else if (xb < pd) {
          for (int l = 0; l < sys.nlayers; l++) {
            const DevLayer &L = sys.layers[l];
            const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
            const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
            int py = y + L.toy + oy; py -= (py >= L.dim) ? L.dim : 0;
            int px = xb + L.tox + ox; px -= (px >= L.dim) ? L.dim : 0;
            add4_ring(ph, base + py * (L.dim + RING_PAD), px, L.dim);
          }
          for (int k = 0; k < sys.ndm; k++) {
            const DevDm &D = sys.dms[k];
            const float *slot = st.dm_shape + (long long)e * sys.shape_stride + D.shape_off;
            const int o = (y + D.toy) * D.dim + xb + D.tox;
            if (D.type == AOMARL_DM_PZT) {
              add4(ph, slot + o);
            } else {
              const float c0 = slot[0], c1 = slot[1];
              float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              add4(f, D.influ + 2 * o);
              add4(f + 4, D.influ + 2 * o + 4);
#pragma unroll
              for (int j = 0; j < 4; j++) ph[j] += c0 * f[2 * j] + c1 * f[2 * j + 1];
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float ar = 0.f, ai = 0.f;
        if (mk[j] != 0.f) {
          float t = ph[j] * sys.tar_inv_lambda;
          t -= rintf(t);
          ar = mk[j] * __builtin_amdgcn_cosf(t);
          ai = mk[j] * __builtin_amdgcn_sinf(t);
          const float d = ph[j] - pivot;
          sd += d; sd2 += d * d; sm += 1.f;
        }
        sar[fy * TGT_TILE_PITCH + fx0 + j] = ar;
        sai[fy * TGT_TILE_PITCH + fx0 + j] = ai;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int xl = 16 * wv + 4 * s + q;
      const float ar = sar[c * TGT_TILE_PITCH + xl], ai = sai[c * TGT_TILE_PITCH + xl];
      const float2 w = tw[(kxf * (x0 + xl)) & (np - 1)];
      Rr = mfma16(ar, w.x, Rr);
      Ri = mfma16(ai, w.x, Ri);
      Rr = mfma16(ai, w.y, Rr);
      Ri = mfma16(ar, -w.y, Ri);
    }
  }
  __syncthreads();
  // cross-wave reduction of the 4 partial tiles; acc reg r of lane (q, c): y = 4q + r, kx = c
#pragma unroll
  for (int r = 0; r < 4; r++) {
    red[(wv * 2 + 0) * 256 + (4 * q + r) * 16 + c] = Rr[r];
    red[(wv * 2 + 1) * 256 + (4 * q + r) * 16 + c] = Ri[r];
  }
  __syncthreads();
  {
    const int yy = tid >> 4, kx = tid & 15;
    if (y0 + yy < pd) {
      float vr = 0.f, vi = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < 4; w4++) { vr += red[(w4 * 2) * 256 + tid]; vi += red[(w4 * 2 + 1) * 256 + tid]; }
      float *o = TR + (((long long)blockIdx.y * pd + (y0 + yy)) * 16 + kx) * 2;
      o[0] = vr; o[1] = vi;
    }
  }
  __syncthreads();
  red[tid] = sd; red[256 + tid] = sd2; red[512 + tid] = sm;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; red[512 + tid] += red[512 + tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float *pp = TPART + ((long long)blockIdx.y * nblk + blockIdx.x) * 4;
    pp[0] = red[0]; pp[1] = red[256]; pp[2] = red[512]; pp[3] = 0.f;
  }
}

// Fast variant (production layout: NL layers, DMs = [stack array, tip-tilt], integer offsets):
// per-environment constants hoisted, all loads of a chunk independent and issued one chunk ahead
// of their use (software pipeline), double-buffered LDS tile -> one barrier per chunk.
template <int NL>
__global__ __launch_bounds__(256) void k_target_rows_fast(DevSys sys, DevState st, int env_begin,
                                                          float *__restrict__ TR,
                                                          float *__restrict__ TPART, int nblk) {
  extern __shared__ float smem[];
  const int pd = sys.pupdiam, np = sys.npsf;
  float *sar = smem;                       // [2][16][65]
  float *sai = sar + 2 * TGT_TILE;
  float *red = sai + 2 * TGT_TILE;          // [4 waves][2][256]
  float2 *stw = reinterpret_cast<float2 *>(red + TGT_RED_MFMA);
  const bool tw_lds = np <= TGT_TW_MAX;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, c = lane & 15;
  const int e = env_begin + blockIdx.y;
  const int y0 = blockIdx.x * 16;
  const float2 *gtw = reinterpret_cast<const float2 *>(sys.psf_tw);
  if (tw_lds)
    for (int j = tid; j < np; j += 256) stw[j] = gtw[j];
  const float2 *tw = tw_lds ? stw : gtw;
  // ---- per-environment constants
  const float *lay[NL];
  int lpx[NL], lpy[NL], ldim[NL];
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const DevLayer &L = sys.layers[l];
    lay[l] = st.screens + (long long)e * sys.screen_stride + L.screen_off;
    ldim[l] = L.dim;
    int px = L.tox + st.origin[(e * sys.nlayers + l) * 2]; px -= (px >= L.dim) ? L.dim : 0;
    int py = L.toy + st.origin[(e * sys.nlayers + l) * 2 + 1]; py -= (py >= L.dim) ? L.dim : 0;
    lpx[l] = px; lpy[l] = py;
  }
  const DevDm &D0 = sys.dms[0], &D1 = sys.dms[1];
  const float *pzt = st.dm_shape + (long long)e * sys.shape_stride + D0.shape_off;
  const float *ttslot = st.dm_shape + (long long)e * sys.shape_stride + D1.shape_off;
  const float c0 = ttslot[0], c1 = ttslot[1];
  const int fy = tid >> 4, fx0 = (tid & 15) * 4;
  const int y = y0 + fy;
  const bool row_ok = y < pd;
  // pivot of the variance sums: phase at the grid centre
  float pivot;
  {
    const int cx = pd / 2, cy = pd / 2;
    float v = pzt[(cy + D0.toy) * D0.dim + cx + D0.tox];
    const float2 f = reinterpret_cast<const float2 *>(D1.influ)[(cy + D1.toy) * D1.dim + cx + D1.tox];
    v += c0 * f.x + c1 * f.y;
#pragma unroll
    for (int l = 0; l < NL; l++) {
      int py = cy + lpy[l]; py -= (py >= ldim[l]) ? ldim[l] : 0;
      int px = cx + lpx[l]; px -= (px >= ldim[l]) ? ldim[l] : 0;
      v += lay[l][py * (ldim[l] + RING_PAD) + px];
    }
    pivot = v;
  }
  // row pointers of this thread
  const float *lrow[NL];
#pragma unroll
  for (int l = 0; l < NL; l++) {
    int py = (row_ok ? y : 0) + lpy[l]; py -= (py >= ldim[l]) ? ldim[l] : 0;
    lrow[l] = lay[l] + py * (ldim[l] + RING_PAD);
  }
  const float *prow = pzt + ((row_ok ? y : 0) + D0.toy) * D0.dim + D0.tox;
  const float *trow = D1.influ + 2 * (((row_ok ? y : 0) + D1.toy) * D1.dim + D1.tox);
  const float *mrow = sys.spupil + (row_ok ? y : 0) * pd;

  float rL[NL][4], rP[4], rT[8], rM[4];
  auto fetch = [&](int x0) {
    const int xb = x0 + fx0;
    const bool ok = row_ok && xb < pd;        // pd % 4 == 0: the 4 columns are in or out together
    const int xs = ok ? xb : 0;
#pragma unroll
    for (int l = 0; l < NL; l++) {
      int px = xs + lpx[l]; px -= (px >= ldim[l]) ? ldim[l] : 0;
      const f4u t = *reinterpret_cast<const f4u *>(lrow[l] + px);
#pragma unroll
      for (int j = 0; j < 4; j++) rL[l][j] = t.v[j];
    }
    const f4u tp = *reinterpret_cast<const f4u *>(prow + xs);
    const f4u t0 = *reinterpret_cast<const f4u *>(trow + 2 * xs);
    const f4u t1 = *reinterpret_cast<const f4u *>(trow + 2 * xs + 4);
    const f4u tm = *reinterpret_cast<const f4u *>(mrow + xs);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      rP[j] = tp.v[j]; rT[j] = t0.v[j]; rT[4 + j] = t1.v[j];
      rM[j] = ok ? tm.v[j] : 0.f;
    }
  };

  f32x4 Rr = {0.f, 0.f, 0.f, 0.f}, Ri = {0.f, 0.f, 0.f, 0.f};
  float sd = 0.f, sd2 = 0.f, sm = 0.f;
  const int kxf = c - 8;
  fetch(0);
  int buf = 0;
  for (int x0 = 0; x0 < pd; x0 += 64, buf ^= 1) {
    float *bar = sar + buf * TGT_TILE, *bai = sai + buf * TGT_TILE;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float ph = rP[j] + (c0 * rT[2 * j] + c1 * rT[2 * j + 1]);
#pragma unroll
      for (int l = 0; l < NL; l++) ph += rL[l][j];
      float ar = 0.f, ai = 0.f;
      if (rM[j] != 0.f) {
        float t = ph * sys.tar_inv_lambda;
        t -= rintf(t);
        ar = rM[j] * __builtin_amdgcn_cosf(t);
        ai = rM[j] * __builtin_amdgcn_sinf(t);
        const float d = ph - pivot;
        sd += d; sd2 += d * d; sm += 1.f;
      }
      bar[fy * TGT_TILE_PITCH + fx0 + j] = ar;
      bai[fy * TGT_TILE_PITCH + fx0 + j] = ai;
    }
    if (x0 + 64 < pd) fetch(x0 + 64);       // next chunk's loads fly during the barrier + MFMAs
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int xl = 16 * wv + 4 * s + q;
      const float ar = bar[c * TGT_TILE_PITCH + xl], ai = bai[c * TGT_TILE_PITCH + xl];
      const float2 w = tw[(kxf * (x0 + xl)) & (np - 1)];
      Rr = mfma16(ar, w.x, Rr);
      Ri = mfma16(ai, w.x, Ri);
      Rr = mfma16(ai, w.y, Rr);
      Ri = mfma16(ar, -w.y, Ri);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; r++) {
    red[(wv * 2 + 0) * 256 + (4 * q + r) * 16 + c] = Rr[r];
    red[(wv * 2 + 1) * 256 + (4 * q + r) * 16 + c] = Ri[r];
  }
  __syncthreads();
  {
    const int yy = tid >> 4, kx = tid & 15;
    if (y0 + yy < pd) {
      float vr = 0.f, vi = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < 4; w4++) { vr += red[(w4 * 2) * 256 + tid]; vi += red[(w4 * 2 + 1) * 256 + tid]; }
      float *o = TR + (((long long)blockIdx.y * pd + (y0 + yy)) * 16 + kx) * 2;
      o[0] = vr; o[1] = vi;
    }
  }
  __syncthreads();
  red[tid] = sd; red[256 + tid] = sd2; red[512 + tid] = sm;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; red[512 + tid] += red[512 + tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float *pp = TPART + ((long long)blockIdx.y * nblk + blockIdx.x) * 4;
    pp[0] = red[0]; pp[1] = red[256]; pp[2] = red[512]; pp[3] = 0.f;
  }
}

// stage 2 on MFMA: G[ky][kx] = sum_y E[ky][y] R[y][kx]; 4 waves split y, one block per env
__global__ __launch_bounds__(256) void k_target_finish_mfma(DevSys sys, const float *__restrict__ TR,
                                                            const float *__restrict__ TPART, int nblk,
                                                            float *__restrict__ PEND,
                                                            uint32_t *__restrict__ frame) {
  __shared__ float red[TGT_RED_MFMA];
  __shared__ double dred[3][64];
  const int pd = sys.pupdiam, np = sys.npsf;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, c = lane & 15;
  const float2 *tw = reinterpret_cast<const float2 *>(sys.psf_tw);
  const float2 *R = reinterpret_cast<const float2 *>(TR) + (long long)b * pd * 16;
  float *pend = PEND + (long long)b * (256 + 4);
  const int kyf = c - 8;
  f32x4 Gr = {0.f, 0.f, 0.f, 0.f}, Gi = {0.f, 0.f, 0.f, 0.f};
  const int per = ((pd + 15) / 16) * 4;              // rows per wave, multiple of 4
  const int yb = wv * per, ye = min(pd, yb + per);
  // 8 steps (32 rows) of operands are fetched before their MFMAs: the loop is latency-bound
  for (int y0 = yb; y0 < ye; y0 += 32) {
    float2 r[8], w[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int y = y0 + 4 * u + q;
      r[u] = make_float2(0.f, 0.f); w[u] = make_float2(0.f, 0.f);
      if (y < ye) {
        r[u] = R[y * 16 + c];                          // B operand: R[y][kx = c]
        w[u] = tw[(kyf * y) & (np - 1)];               // A operand: E[ky = c - 8][y]
      }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      Gr = mfma16(w[u].x, r[u].x, Gr);
      Gi = mfma16(w[u].x, r[u].y, Gi);
      Gr = mfma16(w[u].y, r[u].y, Gr);
      Gi = mfma16(-w[u].y, r[u].x, Gi);
    }
  }
#pragma unroll
  for (int r4 = 0; r4 < 4; r4++) {
    red[(wv * 2 + 0) * 256 + (4 * q + r4) * 16 + c] = Gr[r4];
    red[(wv * 2 + 1) * 256 + (4 * q + r4) * 16 + c] = Gi[r4];
  }
  if (tid < 64) {
    double sd = 0., sd2 = 0., sm = 0.;
    for (int k = tid; k < nblk; k += 64) {
      const float *pp = TPART + ((long long)b * nblk + k) * 4;
      sd += pp[0]; sd2 += pp[1]; sm += pp[2];
    }
    dred[0][tid] = sd; dred[1][tid] = sd2; dred[2][tid] = sm;
  }
  __syncthreads();
  {
    float gr = 0.f, gi = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < 4; w4++) { gr += red[(w4 * 2) * 256 + tid]; gi += red[(w4 * 2 + 1) * 256 + tid]; }
    pend[tid] = gr * gr + gi * gi;                     // tid = ky * 16 + kx
  }
  __syncthreads();
  psf_window_fit(pend, 16);
  if (tid == 0) {
    double sd = 0., sd2 = 0., sm = 0.;
    for (int k = 0; k < 64; k++) { sd += dred[0][k]; sd2 += dred[1][k]; sm += dred[2][k]; }
    double var = 0.;
    if (sm > 0.) { double mean = sd / sm; var = sd2 / sm - mean * mean; }
    pend[256] = (float)var;
    if (frame) frame[b] += 1u;                         // WFS noise frame counter (one-pass path)
  }
}

// publish the pending PSF (strehl_commit_body: aomarl_trace_dev.h)
__global__ __launch_bounds__(256) void k_strehl_commit(DevSys sys, DevState st, int env_begin,
                                                       const float *__restrict__ PEND) {
  strehl_commit_body(sys, st, env_begin, blockIdx.x, PEND);
}

// comp_strehl(do_fit = True), long exposure: the fitted peak of the accumulated window -> slot 7 (on demand:
// aomarl_strehl_fit; one wave per environment)
__global__ __launch_bounds__(64) void k_strehl_fit_le(DevSys sys, DevState st, int env_begin) {
  __shared__ float g2[4];
  const int W = 2 * sys.hw, e = env_begin + blockIdx.x, lane = threadIdx.x;
  float *le = st.le_img + (long long)e * W * W;
  float m = -1.f;
  int arg = 0;
  for (int o = lane; o < W * W; o += 64) { const float v = le[o]; if (v > m) { m = v; arg = o; } }
  for (int d = 32; d >= 1; d >>= 1) {
    const float m2 = __shfl_xor(m, d);
    const int a2 = __shfl_xor(arg, d);
    if (m2 > m || (m2 == m && a2 < arg)) { m = m2; arg = a2; }
  }
  if (lane < 2) g2[lane] = fit_axis_gain(le, W, arg, lane);
  __syncthreads();
  if (lane == 0) {
    float *s = st.strehl + (long long)e * 8;
    s[7] = s[4] > 0.f ? m * g2[0] * g2[1] / s[4] / sys.ref_peak : 0.f;
  }
}

__global__ void k_strehl_reset(DevSys sys, DevState st, int env_begin) {
  const int W = 2 * sys.hw;
  const int e = env_begin + blockIdx.x;
  for (int o = threadIdx.x; o < W * W; o += blockDim.x) st.le_img[(long long)e * W * W + o] = 0.f;
  if (threadIdx.x < 8) st.strehl[(long long)e * 8 + threadIdx.x] = 0.f;
}

// ---------------------------------------------------------------- launchers (aomarl_stage_host.h)
int launch_target_rows(const TargetPlan &p, const DevSys &sys, const DevState &st, int env_begin, float *TR, float *TP,
                       hipStream_t s) {
  const dim3 grid(p.rows_gx, p.rows_gy), blk(p.block);
  switch (p.rows) {
    case ROWS_FAST:
      if (p.nl == 1) hipLaunchKernelGGL(k_target_rows_fast<1>, grid, blk, p.rows_lds, s, sys, st, env_begin, TR, TP, p.nblk);
      else hipLaunchKernelGGL(k_target_rows_fast<3>, grid, blk, p.rows_lds, s, sys, st, env_begin, TR, TP, p.nblk);
      break;
    case ROWS_MFMA:
      if (p.from_buf) hipLaunchKernelGGL(k_target_rows_mfma<true>, grid, blk, p.rows_lds, s, sys, st, env_begin, TR, TP, p.nblk);
      else hipLaunchKernelGGL(k_target_rows_mfma<false>, grid, blk, p.rows_lds, s, sys, st, env_begin, TR, TP, p.nblk);
      break;
    case ROWS_VALU:
      if (p.from_buf) hipLaunchKernelGGL(k_target_rows<true>, grid, blk, p.rows_lds, s, sys, st, env_begin, TR, TP, p.nblk);
      else hipLaunchKernelGGL(k_target_rows<false>, grid, blk, p.rows_lds, s, sys, st, env_begin, TR, TP, p.nblk);
      break;
  }
  LAUNCHCHK();
  return 0;
}

int launch_target_finish(TargetFinish kind, const DevSys &sys, const float *TR, const float *TP, int nblk, float *PEND,
                         uint32_t *frame, int n, hipStream_t s, const FinishEvents *ev) {
  if (kind == FINISH_VALU)
    hipLaunchKernelGGL(k_target_finish, dim3(n), dim3(STAGE_BLOCK), 0, s, sys, TR, TP, nblk, PEND);
  else if (ev)       // (the events ride on the dispatch itself, like the frame kernel's: no marker packets of their own)
    hipExtLaunchKernelGGL(k_target_finish_mfma, dim3(n), dim3(STAGE_BLOCK), 0, s, ev->start, ev->done, 0, sys, TR, TP, nblk,
                          PEND, frame);
  else
    hipLaunchKernelGGL(k_target_finish_mfma, dim3(n), dim3(STAGE_BLOCK), 0, s, sys, TR, TP, nblk, PEND, frame);
  LAUNCHCHK();
  return 0;
}

int launch_strehl_commit(const DevSys &sys, const DevState &st, int env_begin, int n, const float *PEND, hipStream_t s) {
  hipLaunchKernelGGL(k_strehl_commit, dim3(n), dim3(256), 0, s, sys, st, env_begin, PEND);
  LAUNCHCHK();
  return 0;
}
int launch_strehl_reset(const DevSys &sys, const DevState &st, int env_begin, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_strehl_reset, dim3(n), dim3(256), 0, s, sys, st, env_begin);
  LAUNCHCHK();
  return 0;
}
int launch_strehl_fit_le(const DevSys &sys, const DevState &st, int env_begin, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_strehl_fit_le, dim3(n), dim3(64), 0, s, sys, st, env_begin);
  LAUNCHCHK();
  return 0;
}
