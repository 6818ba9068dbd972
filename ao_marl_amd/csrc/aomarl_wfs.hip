// aomarl_wfs.hip -- the staged Shack-Hartmann stage of the environment: spot image and centre of gravity
// (k_wfs_spot, k_wfs_spot_fast), centroids of a stored image cube (k_cog), geometric slopes (k_slopes_geom), and their
// launchers: a translation unit of its own.  It sees the device description (aomarl_dev.h) and a plan
// (aomarl_stage_plan_host.h) through aomarl_stage_host.h, not the context.
#include "aomarl_stage_host.h"
#include "aomarl_trace_dev.h"
#include "aomarl_spot_dev.h"          // add4 .. add4_ring, the spot of one sub-aperture: shared with aomarl_frame.hip

// =============================================================================================
// Shack-Hartmann spot image + centre of gravity.
// One wavefront per (environment, sub-aperture); specialised for the production sampling
// pdiam = 16 phase pixels, Nfft = 64, nrebin = 2, npix = 16 (SURVEY Appendix A / golden fixtures).
//
// The 16x16 complex pupil tile is staged in LDS; the zero-padded 64x64 FFT is never formed:
// only the 32x32 central frequencies feed the 16x16 binned image, and the input has 16 non-zero
// rows/columns, so the transform is the pruned DFT  X = E^T . a . E  with E[16][32] =
// exp(-2 pi i x k / 64), k in [-16, 16): two small complex GEMMs (96 v_mfma_f32_16x16x4_f32).
// |X|^2, the 2x2 binning (binmap), the flux normalisation, optional noise and the COG are done on
// the accumulator registers (spot_compute and what it is made of: aomarl_spot_dev.h).
// =============================================================================================

// phase (sum of all sources) and pupil mask of the 4 pixels this lane owns in sub-aperture i
template <bool FROM_BUF>
__device__ __forceinline__ void spot_load(const DevSys &sys, const DevState &st, int e, int i,
                                          int lane, int no_atmos, int no_dms, float ph[4],
                                          float mk[4]) {
  const int xy0 = sys.sub_xy[i];
  const int gx0 = xy0 & 0xFFFF, gy0 = xy0 >> 16;
  const int ty = lane >> 2, tx0 = (lane & 3) * 4;
  const int gy = gy0 + ty;
#pragma unroll
  for (int j = 0; j < 4; j++) { ph[j] = 0.f; mk[j] = 0.f; }
  if (FROM_BUF) {
    add4(ph, st.wfs_phase + (long long)e * sys.n * sys.n + gy * sys.n + gx0 + tx0);
  } else {
    if (!no_atmos) {
      for (int l = 0; l < sys.nlayers; l++) {
        const DevLayer &L = sys.layers[l];
        const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
        const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
        int py = gy + L.woy + oy; py -= (py >= L.dim) ? L.dim : 0;
        int px = gx0 + tx0 + L.wox + ox; px -= (px >= L.dim) ? L.dim : 0;
        add4_ring(ph, base + py * (L.dim + RING_PAD), px, L.dim);
      }
    }
    if (!no_dms) {
      for (int k = 0; k < sys.ndm; k++) {
        const DevDm &D = sys.dms[k];
        const float *slot = st.dm_shape + (long long)e * sys.shape_stride + D.shape_off;
        const int o = (gy + D.woy) * D.dim + gx0 + tx0 + D.wox;
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
  add4(mk, sys.mpupil + gy * sys.n + gx0 + tx0);
}

// Persistent waves: block = 4 waves, wave w of block bx walks sub-apertures
// (bx*4 + w) + k * gridDim.x*4 of environment blockIdx.y; the phase of the NEXT sub-aperture is
// fetched into registers while the MFMAs of the current one run (hides the load latency chain).
template <bool FROM_BUF, bool NOISE, bool WRITE_CUBE>
__global__ __launch_bounds__(256) void k_wfs_spot(DevSys sys, DevState st, int env_begin,
                                                  int no_atmos, int no_dms, int do_cog) {
  __shared__ float sAr[4][16][17];
  __shared__ float sAi[4][16][17];
  __shared__ float2 sTw[128];                    // (cos, sin)(2 pi m / 128)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e = env_begin + blockIdx.y;
  if (threadIdx.x < 128) {
    float sn, cs;
    sincospif((float)threadIdx.x * (1.0f / 64.0f), &sn, &cs);
    sTw[threadIdx.x] = make_float2(cs, sn);
  }
  __syncthreads();                               // the only block-wide barrier
  const int q = lane >> 4, c = lane & 15;
  const int stride = gridDim.x * 4;
  int i = blockIdx.x * 4 + wv;
  if (i >= sys.nvalid) return;

  // ---- twiddles: idx = 4q + s (pixel), half-integer frequency k + 1/2 with k = c
  float Cc[4], Ss[4];                            // cos / sin(2 pi (2c+1)(4q+s) / 128)
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const float2 w = sTw[((4 * q + s) * (2 * c + 1)) & 127];
    Cc[s] = w.x; Ss[s] = w.y;
  }
  const int ty = lane >> 2, tx0 = (lane & 3) * 4;

  float ph[4], mk[4];
  spot_load<FROM_BUF>(sys, st, e, i, lane, no_atmos, no_dms, ph, mk);
  for (; i < sys.nvalid; i += stride) {
    // ---- stage 0: complex amplitude tile -> LDS (4 pixels per lane)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float t = ph[j] * sys.wfs_inv_lambda;          // revolutions (the half-pixel ramp is folded
                                                     // into the half-integer frequencies)
      t -= rintf(t);
      const float sn = __builtin_amdgcn_sinf(t), cs = __builtin_amdgcn_cosf(t);   // v_sin/v_cos
      sAr[wv][ty][tx0 + j] = mk[j] * cs;
      sAi[wv][ty][tx0 + j] = mk[j] * sn;
    }
    // ---- prefetch the next sub-aperture of this wave
    const int inext = i + stride;
    if (inext < sys.nvalid) spot_load<FROM_BUF>(sys, st, e, inext, lane, no_atmos, no_dms, ph, mk);
    __builtin_amdgcn_wave_barrier();

    spot_compute<NOISE, WRITE_CUBE>(sys, st, e, i, lane, wv, Cc, Ss, sAr, sAi, do_cog, sys.flux[i]);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------------------------------------
// Fast variant for the production layout: NL atmosphere layers, DMs = [stack array, tip-tilt],
// every offset an integer, atmosphere and DMs both seen.  All loads of a tile are independent
// (raw values land in separate registers, the sum is formed at first use), so one wait covers the
// whole prefetch and it overlaps the MFMA block of the previous sub-aperture.  Per-environment
// constants (ring origins, TT commands) are read once per wave.
// ---------------------------------------------------------------------------------------------
template <int NL>
struct SpotEnv {
  const float *lay[NL];
  int px0[NL], py0[NL], dim[NL];
  const float *pzt;
  int pzt_dim, pzt_ox, pzt_oy;
  const float *tt;
  int tt_dim, tt_ox, tt_oy;
  float c0, c1;
};

template <int NL>
struct SpotRaw {
  float L[NL][4];
  float P[4], T[8], M[4];
  float F;   // fluxPerSub of the sub-aperture
};

// All loads of one tile.  Addresses are  uniform base pointer (SGPR) + 32-bit lane offset, so
// the compiler emits global_load ... v_off, s[base] with no 64-bit VALU arithmetic; ring wraps
// cost one v_sub + v_min_u32 per axis (px, px - dim as unsigned: the smaller one is in range).
template <int NL>
__device__ __forceinline__ void spot_fetch(const DevSys &sys, const SpotEnv<NL> &E, int xy0, int ty,
                                           int tx0, int i, SpotRaw<NL> &r) {
  const unsigned gx = (unsigned)((xy0 & 0xFFFF) + tx0), gy = (unsigned)((xy0 >> 16) + ty);
  r.F = sys.flux[i];
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const unsigned dim = (unsigned)E.dim[l];
    unsigned py = gy + (unsigned)E.py0[l]; py = min(py, py - dim);
    unsigned px = gx + (unsigned)E.px0[l]; px = min(px, px - dim);
    const unsigned off = py * (dim + RING_PAD) + px;
    const f4u t = *reinterpret_cast<const f4u *>(E.lay[l] + off);
#pragma unroll
    for (int j = 0; j < 4; j++) r.L[l][j] = t.v[j];
  }
  {
    const unsigned off = (gy + (unsigned)E.pzt_oy) * (unsigned)E.pzt_dim + gx + (unsigned)E.pzt_ox;
    const f4u t = *reinterpret_cast<const f4u *>(E.pzt + off);
#pragma unroll
    for (int j = 0; j < 4; j++) r.P[j] = t.v[j];
  }
  {
    const unsigned off = 2u * ((gy + (unsigned)E.tt_oy) * (unsigned)E.tt_dim + gx + (unsigned)E.tt_ox);
    const f4u t0 = *reinterpret_cast<const f4u *>(E.tt + off);
    const f4u t1 = *reinterpret_cast<const f4u *>(E.tt + off + 4u);
#pragma unroll
    for (int j = 0; j < 4; j++) { r.T[j] = t0.v[j]; r.T[4 + j] = t1.v[j]; }
  }
  {
    const unsigned off = gy * (unsigned)sys.n + gx;
    const f4u t = *reinterpret_cast<const f4u *>(sys.mpupil + off);
#pragma unroll
    for (int j = 0; j < 4; j++) r.M[j] = t.v[j];
  }
}

// stage-1 MFMAs + T combinations of the tile in sAr/sAi (see spot_compute for the algebra)
__device__ __forceinline__ void spot_stage1(int lane, const float (&Cc)[4], const float (&Ss)[4],
                                            const float (*bAr)[17], const float (*bAi)[17],
                                            f32x4 (&Tr)[2], f32x4 (&Ti)[2]) {
  const int q = lane >> 4, c = lane & 15;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 PCr = z4, PCi = z4, PSr = z4, PSi = z4;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const float br = bAr[c][4 * q + s], bi = bAi[c][4 * q + s];
    PCr = mfma16(br, Cc[s], PCr);
    PCi = mfma16(bi, Cc[s], PCi);
    PSr = mfma16(br, Ss[s], PSr);
    PSi = mfma16(bi, Ss[s], PSi);
  }
  Tr[0] = PCr + PSi; Ti[0] = PCi - PSr;
  Tr[1] = PCr - PSi; Ti[1] = PCi + PSr;
}

// Software-pipelined fast kernel.  Per wave and iteration k (tile k of this wave):
//   R1  stage-1 MFMAs of tile k (LDS buffer k&1), T combinations
//   R2  stage-2 MFMAs of tile k  INTERLEAVED (sched_group_barrier) with independent work:
//         amplitude of tile k+1 (sum of the prefetched sources, sin/cos) -> LDS buffer (k+1)&1,
//         address arithmetic + issue of the loads of tile k+2
//   R3  X combinations, |X|^2, binning, COG, store of tile k
// so the VALU / VMEM / LDS-write work of the neighbouring tiles hides under the matrix pipe of
// the current one instead of serialising with it.  The loop body is one basic block (indices are
// clamped instead of branched on).
template <int NL, bool NOISE, bool WRITE_CUBE>
__global__ __launch_bounds__(256) void k_wfs_spot_fast(DevSys sys, DevState st, int env_begin,
                                                       int do_cog) {
  __shared__ float sAr[4][2][16][17];
  __shared__ float sAi[4][2][16][17];
  __shared__ float2 sTw[128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e = env_begin + blockIdx.y;
  if (threadIdx.x < 128) {
    float sn, cs;
    sincospif((float)threadIdx.x * (1.0f / 64.0f), &sn, &cs);
    sTw[threadIdx.x] = make_float2(cs, sn);
  }
  __syncthreads();
  const int q = lane >> 4, c = lane & 15;
  const int stride = gridDim.x * 4;
  const int i0 = blockIdx.x * 4 + wv;
  if (i0 >= sys.nvalid) return;
  const int nit = (sys.nvalid - i0 + stride - 1) / stride;      // tiles of this wave
  const int ilast = i0 + (nit - 1) * stride;
  float Cc[4], Ss[4];                            // cos / sin(2 pi (2c+1)(4q+s) / 128)
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const float2 w = sTw[((4 * q + s) * (2 * c + 1)) & 127];
    Cc[s] = w.x; Ss[s] = w.y;
  }
  const int ty = lane >> 2, tx0 = (lane & 3) * 4;
  const bool owner = (c & 1) == 0;
  // ---- per-environment constants
  SpotEnv<NL> E;
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const DevLayer &L = sys.layers[l];
    E.lay[l] = st.screens + (long long)e * sys.screen_stride + L.screen_off;
    E.dim[l] = L.dim;
    int px = L.wox + st.origin[(e * sys.nlayers + l) * 2]; px -= (px >= L.dim) ? L.dim : 0;
    int py = L.woy + st.origin[(e * sys.nlayers + l) * 2 + 1]; py -= (py >= L.dim) ? L.dim : 0;
    E.px0[l] = px; E.py0[l] = py;
  }
  {
    const DevDm &D0 = sys.dms[0], &D1 = sys.dms[1];
    E.pzt = st.dm_shape + (long long)e * sys.shape_stride + D0.shape_off;
    E.pzt_dim = D0.dim; E.pzt_ox = D0.wox; E.pzt_oy = D0.woy;
    const float *slot = st.dm_shape + (long long)e * sys.shape_stride + D1.shape_off;
    E.c0 = slot[0]; E.c1 = slot[1];
    E.tt = D1.influ; E.tt_dim = D1.dim; E.tt_ox = D1.wox; E.tt_oy = D1.woy;
  }
  const float inv_lambda = sys.wfs_inv_lambda;
  SpotRaw<NL> raw;
  auto amplitude_to_lds = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float ph = raw.P[j] + (E.c0 * raw.T[2 * j] + E.c1 * raw.T[2 * j + 1]);
#pragma unroll
      for (int l = 0; l < NL; l++) ph += raw.L[l][j];
      float t = ph * inv_lambda;
      t -= rintf(t);
      const float sn = __builtin_amdgcn_sinf(t), cs = __builtin_amdgcn_cosf(t);
      sAr[wv][buf][ty][tx0 + j] = raw.M[j] * cs;
      sAi[wv][buf][ty][tx0 + j] = raw.M[j] * sn;
    }
  };
  // ---- prologue: tile 0 -> LDS buffer 0, loads of tile 1 in flight
  spot_fetch<NL>(sys, E, sys.sub_xy[i0], ty, tx0, i0, raw);
  float flux_cur = raw.F;
  amplitude_to_lds(0);
  {
    const int i1 = min(i0 + stride, ilast);
    spot_fetch<NL>(sys, E, sys.sub_xy[i1], ty, tx0, i1, raw);
  }
  int xy2 = sys.sub_xy[min(i0 + 2 * stride, ilast)];
  __builtin_amdgcn_wave_barrier();

  for (int k = 0; k < nit; k++) {
    const int i = i0 + k * stride;
    const int buf = k & 1;
    // ---- R1
    f32x4 Tr[2], Ti[2];
    spot_stage1(lane, Cc, Ss, sAr[wv][buf], sAi[wv][buf], Tr, Ti);
    // ---- R2: stage-2 MFMAs ...
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 Xr[2][2], Xi[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
      f32x4 QCr = z4, QCi = z4, QSr = z4, QSi = z4;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        QCr = mfma16(Cc[s], Tr[m][s], QCr);
        QCi = mfma16(Cc[s], Ti[m][s], QCi);
        QSr = mfma16(Ss[s], Tr[m][s], QSr);
        QSi = mfma16(Ss[s], Ti[m][s], QSi);
      }
      Xr[0][m] = QCr + QSi; Xi[0][m] = QCi - QSr;
      Xr[1][m] = QCr - QSi; Xi[1][m] = QCi + QSr;
    }
    // ... with the neighbours' work: amplitude of tile k+1, loads of tile k+2
    const float flux_next = raw.F;
    amplitude_to_lds(buf ^ 1);
    {
      const int i2 = min(i + 2 * stride, ilast);
      spot_fetch<NL>(sys, E, xy2, ty, tx0, i2, raw);
      xy2 = sys.sub_xy[min(i + 3 * stride, ilast)];
    }
#pragma unroll
    for (int r = 0; r < 32; r++) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // 1 MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);     // 5 VALU
      __builtin_amdgcn_sched_group_barrier(0x220, 1, 0);     // 1 VMEM read or DS write
    }
    // ---- R3: |X|^2, 2x2 binning, flux / COG, store (same mapping as spot_compute)
    float v[2][2][2];
    float tot = 0.f;
#pragma unroll
    for (int sy = 0; sy < 2; sy++)
#pragma unroll
      for (int sx = 0; sx < 2; sx++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
          float a0 = Xr[sy][sx][2 * h], b0 = Xi[sy][sx][2 * h];
          float a1 = Xr[sy][sx][2 * h + 1], b1 = Xi[sy][sx][2 * h + 1];
          float t = (a0 * a0 + b0 * b0) + (a1 * a1 + b1 * b1);
          t = add_xor1(t);
          v[sy][sx][h] = t;
          tot += t;
        }
    const int Xp = 8 + (c >> 1), Xm = 7 - (c >> 1);
    float *sl = st.slopes + (long long)e * sys.nslope;
    if (!NOISE && !WRITE_CUBE) {
      float sx_ = 0.f, sy_ = 0.f;
#pragma unroll
      for (int sy = 0; sy < 2; sy++)
#pragma unroll
        for (int sx = 0; sx < 2; sx++)
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const int Y = sy ? 7 - (2 * q + h) : 8 + 2 * q + h;
            sx_ += v[sy][sx][h] * (float)(sx ? Xm : Xp);
            sy_ += v[sy][sx][h] * (float)Y;
          }
      tot = wave_sum(owner ? tot : 0.f);
      sx_ = wave_sum(owner ? sx_ : 0.f);
      sy_ = wave_sum(owner ? sy_ : 0.f);
      if (do_cog && lane == 0) {
        const float inv = tot > 0.f ? 1.0f / tot : 0.f;
        sl[i] = tot > 0.f ? (sx_ * inv - sys.cog_offset) * sys.cog_scale : 0.f;
        sl[sys.nvalid + i] = tot > 0.f ? (sy_ * inv - sys.cog_offset) * sys.cog_scale : 0.f;
      }
    } else {
      tot = wave_sum(owner ? tot : 0.f);
      const float g = tot > 0.f ? sys.nphot * flux_cur / tot : 0.f;
      float s0 = 0.f, sx = 0.f, sy = 0.f;
      if (NOISE) {
        // lane parity h takes pixel h of each (ty, tx) of the pair's 8 pixels (see spot_finish)
        const int hh = c & 1;
        const uint32_t sd = st.seeds[e], fr = st.frame[e];
#pragma unroll
        for (int ty_ = 0; ty_ < 2; ty_++)
#pragma unroll
          for (int tx_ = 0; tx_ < 2; tx_++) {
            const int Y = ty_ ? 7 - (2 * q + hh) : 8 + 2 * q + hh, X = tx_ ? Xm : Xp;
            const uint32_t idx = (uint32_t)i * 256u + (uint32_t)(Y * 16 + X);
            const float val = sh_noise((hh ? v[ty_][tx_][1] : v[ty_][tx_][0]) * g, sys.noise, sd, fr, idx);
            if (WRITE_CUBE) st.bincube[((long long)e * sys.nvalid + i) * 256 + Y * 16 + X] = val;
            s0 += val;
            sx += val * (float)X;
            sy += val * (float)Y;
          }
      } else {
#pragma unroll
        for (int ty_ = 0; ty_ < 2; ty_++)
#pragma unroll
          for (int tx_ = 0; tx_ < 2; tx_++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
              const int Y = ty_ ? 7 - (2 * q + h) : 8 + 2 * q + h, X = tx_ ? Xm : Xp;
              const float val = v[ty_][tx_][h] * g;
              if (WRITE_CUBE && owner)
                st.bincube[((long long)e * sys.nvalid + i) * 256 + Y * 16 + X] = val;
              s0 += val;
              sx += val * (float)X;
              sy += val * (float)Y;
            }
      }
      if (do_cog) {
        s0 = wave_sum((NOISE || owner) ? s0 : 0.f);
        sx = wave_sum((NOISE || owner) ? sx : 0.f);
        sy = wave_sum((NOISE || owner) ? sy : 0.f);
        if (lane == 0) {
          sl[i] = s0 != 0.f ? (sx / s0 - sys.cog_offset) * sys.cog_scale : 0.f;
          sl[sys.nvalid + i] = s0 != 0.f ? (sy / s0 - sys.cog_offset) * sys.cog_scale : 0.f;
        }
      }
    }
    flux_cur = flux_next;
    __builtin_amdgcn_wave_barrier();
  }
}

// COG from a stored bincube (Rtc.do_centroids on its own): one wave per sub-aperture
__global__ __launch_bounds__(256) void k_cog(DevSys sys, DevState st, int env_begin) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv;
  const int e = env_begin + blockIdx.y;
  if (i >= sys.nvalid) return;
  const int np2 = sys.npix * sys.npix;
  const float *im = st.bincube + ((long long)e * sys.nvalid + i) * np2;
  float s0 = 0.f, sx = 0.f, sy = 0.f;
  for (int p = lane; p < np2; p += 64) {
    float val = im[p];
    int y = p / sys.npix, x = p - y * sys.npix;
    s0 += val; sx += val * (float)x; sy += val * (float)y;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s0 += __shfl_xor(s0, o); sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o);
  }
  if (lane == 0) {
    float *sl = st.slopes + (long long)e * sys.nslope;
    if (s0 != 0.f) {
      sl[i] = (sx / s0 - sys.cog_offset) * sys.cog_scale;
      sl[sys.nvalid + i] = (sy / s0 - sys.cog_offset) * sys.cog_scale;
    } else {
      sl[i] = 0.f; sl[sys.nvalid + i] = 0.f;
    }
  }
}

// geometric slopes from st->wfs_phase (calibration only): one wave per sub-aperture
__global__ __launch_bounds__(256) void k_slopes_geom(DevSys sys, DevState st, int env_begin) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv;
  const int e = env_begin + blockIdx.y;
  if (i >= sys.nvalid) return;
  const int pd = sys.pdiam, n = sys.n;
  const int xy0 = sys.sub_xy[i];
  const int gx0 = xy0 & 0xFFFF, gy0 = xy0 >> 16;
  const float *ph = st.wfs_phase + (long long)e * n * n;
  float gx = 0.f, gyv = 0.f;
  for (int k = lane; k < pd * pd; k += 64) {
    int y = k / pd, x = k - y * pd;
    int xm = x > 0 ? x - 1 : x, xp = x < pd - 1 ? x + 1 : x;
    int ym = y > 0 ? y - 1 : y, yp = y < pd - 1 ? y + 1 : y;
    float m = sys.mpupil[(gy0 + y) * n + gx0 + x];
    float dx = (ph[(gy0 + y) * n + gx0 + xp] - ph[(gy0 + y) * n + gx0 + xm]) / (float)(xp - xm);
    float dy = (ph[(gy0 + yp) * n + gx0 + x] - ph[(gy0 + ym) * n + gx0 + x]) / (float)(yp - ym);
    gx += m * dx; gyv += m * dy;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { gx += __shfl_xor(gx, o); gyv += __shfl_xor(gyv, o); }
  if (lane == 0) {
    const float alpha = 0.206265f / sys.subapd;
    const float den = (float)pd * sys.flux[i];
    float *sl = st.slopes + (long long)e * sys.nslope;
    sl[i] = alpha * gx / den;
    sl[sys.nvalid + i] = alpha * gyv / den;
  }
}

// ---------------------------------------------------------------- launchers (aomarl_stage_host.h)
template <bool FROM_BUF, bool NOISE, bool WRITE_CUBE>
static void spot_generic(const SpotPlan &p, const DevSys &sys, const DevState &st, int env_begin, hipStream_t s) {
  hipLaunchKernelGGL((k_wfs_spot<FROM_BUF, NOISE, WRITE_CUBE>), dim3(p.gx, p.gy), dim3(p.block), 0, s, sys, st, env_begin,
                     p.no_atmos, p.no_dms, p.cog);
}
template <int NL, bool NOISE, bool WRITE_CUBE>
static void spot_fast(const SpotPlan &p, const DevSys &sys, const DevState &st, int env_begin, hipStream_t s) {
  hipLaunchKernelGGL((k_wfs_spot_fast<NL, NOISE, WRITE_CUBE>), dim3(p.gx, p.gy), dim3(p.block), 0, s, sys, st, env_begin, p.cog);
}

int launch_spot(const SpotPlan &p, const DevSys &sys, const DevState &st, int env_begin, hipStream_t s) {
  if (p.refusal != SPOT_OK) return fail("%s", spot_refusal_text(p.refusal));
  const int nc = (p.noise ? 2 : 0) | (p.cube ? 1 : 0);
  if (p.family == SPOT_FAST) {
    switch ((p.nl == 1 ? 0 : 4) | nc) {
      case 0: spot_fast<1, false, false>(p, sys, st, env_begin, s); break;
      case 1: spot_fast<1, false, true>(p, sys, st, env_begin, s); break;
      case 2: spot_fast<1, true, false>(p, sys, st, env_begin, s); break;
      case 3: spot_fast<1, true, true>(p, sys, st, env_begin, s); break;
      case 4: spot_fast<3, false, false>(p, sys, st, env_begin, s); break;
      case 5: spot_fast<3, false, true>(p, sys, st, env_begin, s); break;
      case 6: spot_fast<3, true, false>(p, sys, st, env_begin, s); break;
      default: spot_fast<3, true, true>(p, sys, st, env_begin, s); break;
    }
  } else {
    switch ((p.from_buf ? 4 : 0) | nc) {
      case 0: spot_generic<false, false, false>(p, sys, st, env_begin, s); break;
      case 1: spot_generic<false, false, true>(p, sys, st, env_begin, s); break;
      case 2: spot_generic<false, true, false>(p, sys, st, env_begin, s); break;
      case 3: spot_generic<false, true, true>(p, sys, st, env_begin, s); break;
      case 4: spot_generic<true, false, false>(p, sys, st, env_begin, s); break;
      case 5: spot_generic<true, false, true>(p, sys, st, env_begin, s); break;
      case 6: spot_generic<true, true, false>(p, sys, st, env_begin, s); break;
      default: spot_generic<true, true, true>(p, sys, st, env_begin, s); break;
    }
  }
  LAUNCHCHK();
  return 0;
}

int launch_cog(const DevSys &sys, const DevState &st, int env_begin, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_cog, dim3((sys.nvalid + SPOT_WAVES - 1) / SPOT_WAVES, n), dim3(STAGE_BLOCK), 0, s, sys, st, env_begin);
  LAUNCHCHK();
  return 0;
}

int launch_slopes_geom(const DevSys &sys, const DevState &st, int env_begin, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_slopes_geom, dim3((sys.nvalid + SPOT_WAVES - 1) / SPOT_WAVES, n), dim3(STAGE_BLOCK), 0, s, sys, st, env_begin);
  LAUNCHCHK();
  return 0;
}
