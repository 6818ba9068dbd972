// aomarl_dev.h -- device-side description shared by the kernels of libaomarl_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/aomarl.h"
#include "aomarl_sys.h"      // DevLayer, DevDm, DevSys, RING_PAD

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
// split-fp16 operand pairs (the opt-in fast mode): 2 / 8 halfs, and the matrix instruction they feed
typedef _Float16 hx2 __attribute__((ext_vector_type(2)));
typedef _Float16 hx8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 mfma_h(hx8 a, hx8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

struct DevState {
  int nenv, ld_actu;
  float *screens;
  int32_t *origin;
  uint32_t *seeds, *ext_count;
  float *com, *com1, *com2, *err, *voltage, *slopes, *dm_shape, *bincube, *wfs_phase, *tar_phase;
  float *strehl, *le_img;
  uint32_t *frame;
  float *work;
  int32_t *origin_snap;   // frame pipeline: the kernels that advance a ring origin also write it here (or null)
};

// Sum of split-K slabs in their fixed order with B loads in flight at a time.  Written as a plain loop over a run-time
// count, the compiler emits load / wait / add per slab: every slab costs a full load latency (4 us of the 18 us
// scatter + gather launch inside the reset, one to two microseconds per slab in the chains' consumers beside the
// frame kernel).  at(z): the z-th slab's element (slabs past the count re-read the last one and are not added).
template <int B, typename F>
__device__ __forceinline__ float slab_sum(int nsplit, F at) {
  float acc = 0.f;
  for (int z0 = 0; z0 < nsplit; z0 += B) {
    float pz[B];
#pragma unroll
    for (int z = 0; z < B; z++) pz[z] = at(min(z0 + z, nsplit - 1));
#pragma unroll
    for (int z = 0; z < B; z++) acc = (z0 + z < nsplit) ? acc + pz[z] : acc;
  }
  return acc;
}

// ---------------------------------------------------------------- Philox4x32-10 + normals
// (same definition as the oracle: key = {seed, "AOMR"}, ctr = {block, counter_lo, counter_hi,
//  stream}; 4 outputs -> 4 uniforms or 2 Box-Muller pairs)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
  // both halves of a 32 x 32 product from ONE instruction (v_mad_u64_u32: 6.5 cycles of the SIMD against 5.2 + 5.5 for
  // v_mul_hi_u32 + v_mul_lo_u32 with three waves resident, tools/valubench.hip); the multiplier rides in a scalar
  // register (VOP3 takes no 32-bit literal on this target)
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    uint64_t m0, m1;
    asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(m0) : "s"(M0), "v"(c0) : "vcc");
    asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(m1) : "s"(M1), "v"(c2) : "vcc");
    const uint32_t hi0 = (uint32_t)(m0 >> 32), lo0 = (uint32_t)m0, hi1 = (uint32_t)(m1 >> 32), lo1 = (uint32_t)m1;
    uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float u01(uint32_t x) {
  return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f);
}

// elements 4 j .. 4 j + 3 of the normal stream (seed, stream, counter): the four of them come out of
// one Philox block and two Box-Muller pairs (same values as philox_normal element by element)
__device__ __forceinline__ void philox_normal4(uint32_t seed, uint32_t stream, uint32_t cnt_lo,
                                               uint32_t cnt_hi, uint32_t j, float out[4]) {
  uint32_t x[4];
  philox4x32_10(j, cnt_lo, cnt_hi, stream, seed, 0x414F4D52u, x);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float u0 = u01(x[2 * h]), u1 = u01(x[2 * h + 1]);
    const float r = sqrtf(-2.0f * logf(u0));
    const float a = 6.28318530717958647692f * u1;
    out[2 * h] = r * cosf(a);
    out[2 * h + 1] = r * sinf(a);
  }
}

// element `idx` of the normal stream (seed, stream, counter)
__device__ __forceinline__ float philox_normal(uint32_t seed, uint32_t stream, uint32_t cnt_lo,
                                               uint32_t cnt_hi, uint32_t idx) {
  uint32_t x[4];
  philox4x32_10(idx >> 2, cnt_lo, cnt_hi, stream, seed, 0x414F4D52u, x);
  int h = (idx >> 1) & 1;
  float u0 = u01(x[2 * h]), u1 = u01(x[2 * h + 1]);
  float r = sqrtf(-2.0f * logf(u0));
  float a = 6.28318530717958647692f * u1;
  return (idx & 1) ? r * sinf(a) : r * cosf(a);
}

__device__ __forceinline__ float poisson_draw(float lam, float u, float zn) {
  if (!(lam > 0.f)) return 0.f;
  if (lam < 30.f) {
    // hardware exp2 / reciprocal (1 ulp): the cumulative sums move in their last bit against the
    // oracle's libm, which flips a count where u sits within ~1e-7 of a threshold
    float p = __expf(-lam), c = p;
    int k = 0;
    // the fp32 cumulative sum levels off a few ulps below 1 (0.9999999 for lam = 1) while u01 reaches 1.0: for a u
    // above that level `u > c` never fails and the count would run to the cap (200 photons in a dark pixel, ~1e-7 of
    // the pixels, at different u on the two sides).  Stop where the sum stops growing: the count there is the tail's end
    while (u > c && k < 200) {
      k++;
      p *= lam * __builtin_amdgcn_rcpf((float)k);
      const float cn = c + p;
      if (cn == c) break;
      c = cn;
    }
    return (float)k;
  }
  float v = floorf(lam + sqrtf(lam) * zn + 0.5f);
  return v < 0.f ? 0.f : v;
}

// photon + read noise of one pixel: ONE Philox block per (pixel, frame) -- word 0: uniform of the
// Poisson inversion, words 1, 2: a Box-Muller pair (cosine branch: rounded-normal Poisson for
// lam >= 30, sine branch: read noise).  Same rule as oracle/aoref.c:aoref_sh_noise.
__device__ __forceinline__ float sh_noise(float lam, float sigma, uint32_t seed, uint32_t frame, uint32_t idx) {
  uint32_t x[4];
  philox4x32_10(idx, frame, 0u, 4u, seed, 0x414F4D52u, x);
  // Box-Muller on the transcendental unit: log2, and sin / cos of an angle given in revolutions
  // (v_sin_f32 / v_cos_f32 take exactly that) -- ~6 instructions against ~150 for libm's logf, sinf,
  // cosf; the normals agree with the oracle's to ~1e-6
  const float r = sqrtf(-2.0f * __logf(u01(x[1])));
  const float t = u01(x[2]);
  float v = poisson_draw(lam, u01(x[0]), r * __builtin_amdgcn_cosf(t));
  if (sigma > 0.f) v += sigma * (r * __builtin_amdgcn_sinf(t));
  return v;
}

// ring-buffered screen: logical (x, y) -> physical float index.  Physical rows are
// n + RING_PAD floats long: columns [n, n + RING_PAD) mirror columns [0, RING_PAD), so up to
// RING_PAD consecutive logical pixels starting at a physical column < n are consecutive floats:
// a 16-pixel tile row whose first pixel is in range needs no wrap test per lane (the one-pass
// frame kernel wraps once per tile -- once per PAIR of tiles, 32 pixels, when it fetches whole 128-byte row
// pieces -- on the scalar unit); the extrusion scatter keeps the mirror up to date.
// (RING_PAD: aomarl_sys.h)
__device__ __forceinline__ int ring_idx(int x, int y, int ox, int oy, int n) {
  int px = x + ox;
  px -= (px >= n) ? n : 0;
  int py = y + oy;
  py -= (py >= n) ? n : 0;
  return py * (n + RING_PAD) + px;
}

// Dynamic LDS of a k_frame_wave workgroup: byte offsets of its regions and their sum.  The kernel takes its pointers
// from this, the host the size of the launch.
//   0      [128] float2 WFS twiddles (none in the slopes-only fp32 instantiation, qf)
//   lat    [4 waves][4 NB][latw] floats: the command lattice (stack-array DM from the voltages, otf)
//   slots  the block's shared-data slots -- per-tile walk: [2][4][64] float4; pair walk: [2 parities][2 tiles][4][64]
//   img    otf: [4 waves][NL] images of a tile pair's layer rows, FWD_IMG bytes each; otherwise 128 bytes of slack
//   qmom   qf: [4 waves][ntl] float4 moments of the stripe's sub-apertures
#define FWD_IMG (2 * 1024 + 128)           // bytes of a layer image
struct FrameLds { int lat, slots, img, qmom, total; };
__host__ __device__ constexpr FrameLds frame_lds(bool qf, bool otf, int NL, int NB, int latw, int ntl) {
  const int lat = qf ? 0 : 128 * 8;
  const int slots = lat + 4 * (4 * 4 * NB * (otf ? latw : 0));
  const int img = slots + 16384;
  const int qmom = img + (otf ? 4 * NL * FWD_IMG : 128);
  return {lat, slots, img, qmom, qmom + (qf ? 4 * 16 * ntl : 0)};
}

// ---- cross-lane helpers on the VALU (DPP) instead of the LDS crossbar (ds_bpermute)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// v + v[lane ^ 1]
__device__ __forceinline__ float add_xor1(float v) { return v + dpp_f<0xB1>(v); }   // quad_perm [1,0,3,2]
// sum over the 64 lanes, result uniform (returned in every lane)
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f<0xB1>(v);      // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);      // quad_perm [2,3,0,1]
  v += dpp_f<0x124>(v);     // row_ror:4
  v += dpp_f<0x128>(v);     // row_ror:8   -> every lane holds its 16-lane row sum
  return (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) +
          __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)) +
          __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48)));
}

// sum over the 64 lanes, valid in LANE 63 ONLY: 6 DPP adds, no v_readlane (row_bcast:15 / :31 carry
// the row sums across the four 16-lane rows)
__device__ __forceinline__ float wave_sum_last(float v) {
  v += dpp_f<0xB1>(v);      // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);      // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);     // row_half_mirror
  v += dpp_f<0x140>(v);     // row_mirror -> every lane holds its 16-lane row sum
  // rows 1, 3 += last lane of the row before; rows 2, 3 += last lane of row 1: ONE instruction each
  // (dst == src, the rows the mask leaves out keep their value) -- written through update_dpp with a
  // zero `old` the compiler needs v_mov 0 + v_mov_dpp + v_add per step
  asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(v));
  asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(v));
  return v;
}
