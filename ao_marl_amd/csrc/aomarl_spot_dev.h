// aomarl_spot_dev.h -- the device functions the one-pass frame kernel (aomarl_frame.hip) shares with the environment's
// other kernels (aomarl_wfs.hip: k_wfs_spot, k_wfs_spot_fast; aomarl_target.hip: the target kernels; aomarl_kernels.hip:
// aomarl_gemm_nt.h): the split-fp16 operand helpers, the unaligned 4-float loads and the Shack-Hartmann spot of one
// sub-aperture on the matrix cores.  Each is the one text every unit compiles.
#pragma once
#include "aomarl_dev.h"

// ---- split-fp16 helpers (used by the loop's GEMM, aomarl_gemm_nt.h, and by the frame kernel; see the frame kernel's notes)
// (hx2 / hx8 and mfma_h: aomarl_dev.h -- the denoiser's translation unit uses them too)

__device__ __forceinline__ hx2 cvt_h2(float a, float b) {
  return __builtin_bit_cast(hx2, __builtin_amdgcn_cvt_pkrtz(a, b));
}
// a - f32(h.lo) and a - f32(h.hi) as single mixed-precision FMAs (v_fma_mix_f32 reads the f16 half
// directly; the compiler will not form it from a - (float)h).  Operands always come out of ordinary
// VALU instructions (v_cvt_pkrtz of the same value sits in between any producer and this read).
__device__ __forceinline__ float sub_lo(hx2 h, float a) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(a));
  return r;
}
__device__ __forceinline__ float sub_hi(hx2 h, float a) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(a));
  return r;
}

// 4 consecutive floats at a dword-aligned (not necessarily 16-byte aligned) address: one
// global_load_dwordx4 (gfx950 supports unaligned vector access; the compiler emits it for this type)
struct __attribute__((packed, aligned(4))) f4u { float v[4]; };
__device__ __forceinline__ void add4(float acc[4], const float *p) {
  const f4u t = *reinterpret_cast<const f4u *>(p);
  acc[0] += t.v[0]; acc[1] += t.v[1]; acc[2] += t.v[2]; acc[3] += t.v[3];
}
// 4 consecutive logical pixels of a ring-buffered screen row starting at physical column px
__device__ __forceinline__ void add4_ring(float acc[4], const float *row, int px, int dim) {
  (void)dim;                     // rows carry RING_PAD mirror columns: never wraps
  add4(acc, row + px);
}

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// An all-zero accumulator the compiler cannot rematerialise: MFMAs that start a chain read it as
// their C operand (dst != srcC form) instead of zero-filling a fresh accumulator with v_mov each
// time (fp32 MFMAs and VALU instructions share the issue slots, so every v_mov counts).
__device__ __forceinline__ f32x4 opaque_zero4() {
  float z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  f32x4 r = {z, z, z, z};
  return r;
}

// (poisson_draw and sh_noise, the draw rule of a pixel, live in aomarl_dev.h: the pyramid sensor shares them)

// MFMA stages + binning + normalisation (+noise) + COG of one sub-aperture whose complex amplitude
// tile b = mask * exp(i phi 2pi/lambda) is in sAr/sAi[wv]; shared by the generic and fast kernels.
//
// The 32 kept frequencies [-16, 15] of the 64-point transform of  a = b * exp(-i pi (x+y)/64)
// (the reference's half-pixel ramp `halfxy`, geom_init.py:689-701) are the HALF-INTEGER
// frequencies kappa = +-(k + 1/2), k = 0..15, of b itself:  kx = k  <->  +(k+1/2),
// kx = -(k+1)  <->  -(k+1/2).  The +- pairs share cos and differ in the sign of sin, so with
//   C[x][k] = cos(2 pi (2k+1) x / 128),  S[x][k] = sin(2 pi (2k+1) x / 128)      (16 x 16, real)
// stage 1 needs the 4 real products  b_r C, b_i C, b_r S, b_i S  (16 MFMAs) and gives both
// T+ = (PCr + PSi, PCi - PSr) and T- = (PCr - PSi, PCi + PSr); stage 2 does the same along y for
// T+ and T- (32 MFMAs): 48 v_mfma_f32_16x16x4_f32 instead of 96 for the plain complex products.
// Accumulator layout of stage 1 (row y = 4q + reg, col k = c) is again exactly the B-operand
// K-order stage 2 wants, and the twiddle registers serve as B operand (stage 1) and A operand
// (stage 2) alike, so nothing moves between the stages.
// ---------------------------------------------------------------------------------------------
// Split-fp16 operands for the real matrix cores.  v_mfma_f32_16x16x32_f16 costs 16 cycles against
// the 4 x 32 of the four fp32 MFMAs it replaces (fp32 MFMAs run at the vector rate).
// A value v is carried as hi = f16(v), lo = f16(v - hi): 22 mantissa bits.  The K = 32 slots of
// one instruction hold the 16 real terms twice, so
//     mfma(pack(a), dup_hi(b)) + mfma(pack(a), dup_lo(b))     with pack(a) = [a_hi | a_lo]
// is the full (a_hi + a_lo)(b_hi + b_lo) product, accumulated in fp32.  Lane (q, c) owns the 4
// values (row c, k = 4q .. 4q+3) of an operand -- for the amplitude tile those are exactly the 4
// pixels the lane computed, and for stage 2 exactly its 4 accumulator registers of stage 1: no LDS.
// ---------------------------------------------------------------------------------------------
// [hi(a0..a3) | lo(a0..a3)]
__device__ __forceinline__ hx8 pack_hl(float a0, float a1, float a2, float a3) {
  const hx2 h01 = cvt_h2(a0, a1), h23 = cvt_h2(a2, a3);
  const hx2 l01 = cvt_h2(sub_lo(h01, a0), sub_hi(h01, a1));
  const hx2 l23 = cvt_h2(sub_lo(h23, a2), sub_hi(h23, a3));
  return hx8{h01[0], h01[1], h23[0], h23[1], l01[0], l01[1], l23[0], l23[1]};
}
// [hi | hi] and [lo | lo]
__device__ __forceinline__ void dup_hl(float a0, float a1, float a2, float a3, hx8 &H, hx8 &L) {
  const hx2 h01 = cvt_h2(a0, a1), h23 = cvt_h2(a2, a3);
  const hx2 l01 = cvt_h2(sub_lo(h01, a0), sub_hi(h01, a1));
  const hx2 l23 = cvt_h2(sub_lo(h23, a2), sub_hi(h23, a3));
  H = hx8{h01[0], h01[1], h23[0], h23[1], h01[0], h01[1], h23[0], h23[1]};
  L = hx8{l01[0], l01[1], l23[0], l23[1], l01[0], l01[1], l23[0], l23[1]};
}
// twiddle operands of the spot DFT in split-fp16 form (constant per lane)
struct SpotTwH { hx8 CH, CL, SH, SL; };
__device__ __forceinline__ SpotTwH spot_tw_h(const float (&Cc)[4], const float (&Ss)[4]) {
  SpotTwH t;
  dup_hl(Cc[0], Cc[1], Cc[2], Cc[3], t.CH, t.CL);
  dup_hl(Ss[0], Ss[1], Ss[2], Ss[3], t.SH, t.SL);
  return t;
}

// the two DFT stages on fp32 MFMAs: br[s] / bi[s] = complex amplitude of pixel (y = c, x = 4q + s)
__device__ __forceinline__ void spot_dft_f32(const float (&Cc)[4], const float (&Ss)[4],
                                             const float (&br)[4], const float (&bi)[4],
                                             const f32x4 z4, f32x4 (&Xr)[2][2], f32x4 (&Xi)[2][2]) {
  // ---- stage 1 (y = c on M, x = 4q + s on K, k = c on N)
  f32x4 PCr = z4, PCi = z4, PSr = z4, PSi = z4;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    PCr = mfma16(br[s], Cc[s], PCr);
    PCi = mfma16(bi[s], Cc[s], PCi);
    PSr = mfma16(br[s], Ss[s], PSr);
    PSi = mfma16(bi[s], Ss[s], PSi);
  }
  f32x4 Tr[2], Ti[2];                 // [0]: kx = +(k+1/2)   [1]: kx = -(k+1/2)
  Tr[0] = PCr + PSi; Ti[0] = PCi - PSr;
  Tr[1] = PCr - PSi; Ti[1] = PCi + PSr;
  // ---- stage 2 (ky' = c on M, y = 4q + s on K = accumulator reg s, kx' on N)
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
}

// |X|^2 and 2x2 binning of one quadrant tile.  Reg r, lane (q, c): ky' = 4q + r, kx' = c;
// + tiles: k = k' -> LR index 8 + (k' >> 1);  - tiles: k = -(k'+1) -> LR index 7 - (k' >> 1)
__device__ __forceinline__ void spot_bin(const f32x4 Xr, const f32x4 Xi, float (&v)[2]) {
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float a0 = Xr[2 * h], b0 = Xi[2 * h], a1 = Xr[2 * h + 1], b1 = Xi[2 * h + 1];
    v[h] = add_xor1((a0 * a0 + b0 * b0) + (a1 * a1 + b1 * b1));
  }
}

// the split-fp16 DFT with the binning folded in per kx-sign half: only 2 of the 4 quadrant tiles
// are ever live (32 accumulator registers instead of 64)
__device__ __forceinline__ void spot_dft_h_v(const SpotTwH &tw, const float (&br)[4],
                                             const float (&bi)[4], const f32x4 z4,
                                             float (&v)[2][2][2]) {
  const hx8 ar = pack_hl(br[0], br[1], br[2], br[3]), ai = pack_hl(bi[0], bi[1], bi[2], bi[3]);
  f32x4 PCr = mfma_h(ar, tw.CL, mfma_h(ar, tw.CH, z4));
  f32x4 PCi = mfma_h(ai, tw.CL, mfma_h(ai, tw.CH, z4));
  f32x4 PSr = mfma_h(ar, tw.SL, mfma_h(ar, tw.SH, z4));
  f32x4 PSi = mfma_h(ai, tw.SL, mfma_h(ai, tw.SH, z4));
#pragma unroll
  for (int m = 0; m < 2; m++) {                // [0]: kx = +(k+1/2)   [1]: kx = -(k+1/2)
    const f32x4 Tr = m == 0 ? PCr + PSi : PCr - PSi;
    const f32x4 Ti = m == 0 ? PCi - PSr : PCi + PSr;
    const hx8 tr = pack_hl(Tr[0], Tr[1], Tr[2], Tr[3]);
    const hx8 ti = pack_hl(Ti[0], Ti[1], Ti[2], Ti[3]);
    const f32x4 QCr = mfma_h(tw.CL, tr, mfma_h(tw.CH, tr, z4));
    const f32x4 QCi = mfma_h(tw.CL, ti, mfma_h(tw.CH, ti, z4));
    const f32x4 QSr = mfma_h(tw.SL, tr, mfma_h(tw.SH, tr, z4));
    const f32x4 QSi = mfma_h(tw.SL, ti, mfma_h(tw.SH, ti, z4));
    // X(+ky) = (QCr + QSi, QCi - QSr), X(-ky) = (QCr - QSi, QCi + QSr):
    //   |X(+-ky)|^2 = P +- 2 D,  P = QCr^2 + QSi^2 + QCi^2 + QSr^2,  D = QCr QSi - QCi QSr
    // and the 2 x 2 binning adds register pairs (2h, 2h + 1) and lane pairs (c, c ^ 1): P and D are
    // summed over the register pair first (14 instructions per pair for both signs instead of 20)
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int a = 2 * h, b = 2 * h + 1;
      float P = QCr[a] * QCr[a];
      P = fmaf(QSi[a], QSi[a], P); P = fmaf(QCi[a], QCi[a], P); P = fmaf(QSr[a], QSr[a], P);
      P = fmaf(QCr[b], QCr[b], P); P = fmaf(QSi[b], QSi[b], P); P = fmaf(QCi[b], QCi[b], P); P = fmaf(QSr[b], QSr[b], P);
      float D = QCr[a] * QSi[a];
      D = fmaf(-QCi[a], QSr[a], D); D = fmaf(QCr[b], QSi[b], D); D = fmaf(-QCi[b], QSr[b], D);
      v[0][m][h] = add_xor1(fmaf(2.f, D, P));
      v[1][m][h] = add_xor1(fmaf(-2.f, D, P));
    }
  }
}

// Slopes only (no noise, no image wanted), fp32: the centre of gravity straight from the stage-2 products.
// With X(+-ky) = (QCr +- QSi, QCi -+ QSr):  |X(+-ky)|^2 = P +- 2 D,  P = QCr^2 + QSi^2 + QCi^2 + QSr^2,
// D = QCr QSi - QCi QSr.  The image is never formed: the 2 x 2 binning only gives pairs of frequencies the same
// pixel coordinate, so the three moments are weighted sums of P and D with per-lane constants --
//   pixel row of +ky: 8 + 2q + (r >> 1), of -ky: 7 - 2q - (r >> 1): their sum is 15, their difference
//   1 + 4q + 2 (r >> 1); pixel column of +kx: Xp = 8 + (c >> 1), of -kx: Xm = 7 - (c >> 1) --
//   sum I   = 2 (P0 + P1)                    (Pm: P summed over the lane's 4 registers of half m)
//   sum x I = 2 (Xp P0 + Xm P1)
//   sum y I = 15 (P0 + P1) + 2 [(1 + 4q) (D over r = 0, 1) + (3 + 4q) (D over r = 2, 3)]
// (the common factor 2 drops out of the ratios): 48 multiply-adds + 8 for the moments, against 125 vector
// instructions for combine / square / bin / weight -- on fp32 matrix instructions vector and matrix work
// share the issue slots, so every one of them is kernel time.
__device__ __forceinline__ void spot_cog_f32(const DevSys &sys, const DevState &st, int e, int i, int lane,
                                             const float (&Cc)[4], const float (&Ss)[4], const float (&br)[4],
                                             const float (&bi)[4], int do_cog, const f32x4 z4) {
  const int q = lane >> 4, c = lane & 15;
  // ---- stage 1 (y = c on M, x = 4q + s on K, k = c on N)
  f32x4 PCr = z4, PCi = z4, PSr = z4, PSi = z4;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    PCr = mfma16(br[s], Cc[s], PCr);
    PCi = mfma16(bi[s], Cc[s], PCi);
    PSr = mfma16(br[s], Ss[s], PSr);
    PSi = mfma16(bi[s], Ss[s], PSi);
  }
  float Pm[2], Da = 0.f, Db = 0.f;
#pragma unroll
  for (int m = 0; m < 2; m++) {                  // [0]: kx = +(k+1/2)   [1]: kx = -(k+1/2)
    const f32x4 Tr = m == 0 ? PCr + PSi : PCr - PSi;
    const f32x4 Ti = m == 0 ? PCi - PSr : PCi + PSr;
    f32x4 QCr = z4, QCi = z4, QSr = z4, QSi = z4;
#pragma unroll
    for (int s = 0; s < 4; s++) {
      QCr = mfma16(Cc[s], Tr[s], QCr);
      QCi = mfma16(Cc[s], Ti[s], QCi);
      QSr = mfma16(Ss[s], Tr[s], QSr);
      QSi = mfma16(Ss[s], Ti[s], QSi);
    }
    float P = QCr[0] * QCr[0];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (r) P = fmaf(QCr[r], QCr[r], P);
      P = fmaf(QSi[r], QSi[r], P); P = fmaf(QCi[r], QCi[r], P); P = fmaf(QSr[r], QSr[r], P);
    }
    Pm[m] = P;
    Da = fmaf(QCr[0], QSi[0], Da); Da = fmaf(-QCi[0], QSr[0], Da);
    Da = fmaf(QCr[1], QSi[1], Da); Da = fmaf(-QCi[1], QSr[1], Da);
    Db = fmaf(QCr[2], QSi[2], Db); Db = fmaf(-QCi[2], QSr[2], Db);
    Db = fmaf(QCr[3], QSi[3], Db); Db = fmaf(-QCi[3], QSr[3], Db);
  }
  const float Xp = (float)(8 + (c >> 1)), Xm = (float)(7 - (c >> 1));
  float s0 = Pm[0] + Pm[1];
  float sx = fmaf(Xm, Pm[1], Xp * Pm[0]);
  float sy = fmaf((float)(3 + 4 * q), Db, fmaf((float)(1 + 4 * q), Da, 7.5f * s0));
  s0 = wave_sum_last(s0);
  sx = wave_sum_last(sx);
  sy = wave_sum_last(sy);
  if (do_cog && lane == 63) {
    float *sl = st.slopes + (long long)e * sys.nslope;
    if (s0 > 0.f) {
      const float inv = __builtin_amdgcn_rcpf(s0);       // 1 ulp; slopes are compared at 1e-4"
      sl[i] = (sx * inv - sys.cog_offset) * sys.cog_scale;
      sl[sys.nvalid + i] = (sy * inv - sys.cog_offset) * sys.cog_scale;
    } else {
      sl[i] = 0.f;
      sl[sys.nvalid + i] = 0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Packed fp32 vector arithmetic, hand-emitted.  On this chip fp32 matrix instructions run at the PACKED-fp32
// vector rate and share the issue slots with the vector unit, so a v_pk_fma_f32 does twice
// the work of a v_fma_f32 for the same 4 issue cycles -- but the compiler's pre-emit peephole splits packed fp32
// operations that follow matrix instructions back into scalar ones (it assumes a separate matrix pipe), and the
// vector work of the frame kernel sits exactly there.  Inline asm keeps them packed.  The price: the compiler's
// hazard recogniser does not look inside inline asm, so the software-visible wait states of gfx950 are kept BY
// HAND -- a result of v_mfma_f32_16x16x4_f32 (8 passes) must not be read by a vector instruction for 10 wait
// states, a transcendental's result not by a non-transcendental for 1: every group of packed instructions whose
// inputs come from matrix or transcendental instructions opens with PK_GUARD_*: a scheduling barrier (everything
// written before it in the source is issued before it) and an s_nop that covers the longest such distance.
// All statements are `asm volatile`: they stay in source order among themselves.
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define PK_GUARD_MFMA() do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_nop 10"); } while (0)
#define PK_GUARD_TRANS() do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_nop 1"); } while (0)
// (a group's results feed matrix instructions: two wait states of margin, although gfx950 documents none)
#define PK_END_TO_MFMA() do { asm volatile("s_nop 1"); __builtin_amdgcn_sched_barrier(0); } while (0)
__device__ __forceinline__ f32x2 pk_lo(f32x4 v) { return __builtin_shufflevector(v, v, 0, 1); }
__device__ __forceinline__ f32x2 pk_hi(f32x4 v) { return __builtin_shufflevector(v, v, 2, 3); }
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
  f32x2 d;
  asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ f32x2 pk_mul(f32x2 a, f32x2 b) {
  f32x2 d;
  asm volatile("v_pk_mul_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// in-place forms for accumulators that live across branches / loop iterations (an "=v" result is a new register: the
// compiler then copies it back where control flow joins) and forms whose constant operand stays in a scalar register
// pair (a loop-invariant pair in vector registers is re-materialised from its scalars every iteration: one
// v_mov_b64 each; a packed instruction may read one scalar pair)
__device__ __forceinline__ void pk_acc_add(f32x2 &acc, f32x2 x) { asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(acc) : "v"(x)); }
__device__ __forceinline__ void pk_acc_fma(f32x2 &acc, f32x2 a, f32x2 b) { asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b)); }
// acc -= a * b
__device__ __forceinline__ void pk_acc_fnma(f32x2 &acc, f32x2 a, f32x2 b) {
  asm volatile("v_pk_fma_f32 %0, %1, %2, %0 neg_lo:[1,0,0] neg_hi:[1,0,0]" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ f32x2 pk_fma_s(f32x2 a, f32x2 bs, f32x2 c) {
  f32x2 d;
  asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(bs), "v"(c));
  return d;
}
__device__ __forceinline__ f32x2 pk_fma_nc_s(f32x2 a, f32x2 bs, f32x2 c) {
  f32x2 d;
  asm volatile("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(d) : "v"(a), "s"(bs), "v"(c));
  return d;
}
__device__ __forceinline__ f32x2 pk_mul_s(f32x2 a, f32x2 bs) {
  f32x2 d;
  asm volatile("v_pk_mul_f32 %0, %1, %2" : "=v"(d) : "v"(a), "s"(bs));
  return d;
}

// ---------------------------------------------------------------------------------------------
// Slopes only, fp32, WITHOUT the spot: the three moments of the binned image as quadratic forms of the
// pupil field (16 matrix instructions per sub-aperture -- four 16 x 16 x 16 products -- instead of the transform's 48).
//
// The binned image covers the central 32 x 32 frequencies f = +-(j + 1/2), j = 0 .. 15 of the half-pixel-shifted
// 64-point transform, every one of them exactly once (npix * nrebin = 32), and the pixel coordinate of a frequency
// depends on one axis only: X(+-(j + 1/2)) = 7.5 +- u_j, u_j = 1/2 + (j >> 1).  A sum  sum_f w_x(fx) w_y(fy) |F(fx, fy)|^2
// with F = sum_{x, y} E[y][x] exp(-2 pi i (fx x + fy y) / 64) is then
//     sum_{x, x', y, y'} E[y][x] conj(E[y'][x']) K_wx[x'][x] K_wy[y'][y],    K_w[x'][x] = sum_f w(f) exp(2 pi i f (x' - x) / 64),
// and for w = 1 the kernel is the real symmetric Toeplitz matrix  M[d] = 2 sum_j cos(2 pi (j + 1/2) d / 64), for the
// odd weight w = +-u_j it is i S with  S[d] = 2 sum_j u_j sin(2 pi (j + 1/2) d / 64)  real and antisymmetric.  With
// E = Er + i Ei (rows y, columns x) the imaginary parts cancel and
//     sum I           = < M, Er M Er^T + Ei M Ei^T >
//     sum (X - 7.5) I =  2 < M, Ei S Er^T >
//     sum (Y - 7.5) I =  2 < S, Ei M Er^T >            (< A, B > = sum_{y', y} A[y'][y] B[y'][y])
// Both kernels factor through ONE real 16-column basis (aomarl_qf4_host.h builds it on the host, in double):
//     M = H' H'^T,      S = H' L H'^T,      L = 2 x 2 blocks [[0, t_k], [-t_k, 0]] on eight pairs of columns,
// so that with  P = H'^T E H' = Pr + i Pi  (complex 16 x 16: rows b belong to y, columns a to x)
//     sum I           = |Pr|^2 + |Pi|^2
//     sum (X - 7.5) I = 2 sum_b sum_k t_k (Pi[b][k] Pr[b][k'] - Pi[b][k'] Pr[b][k])      (k, k': the columns of pair k)
//     sum (Y - 7.5) I = 2 sum_a sum_k t_k (Pi[k][a] Pr[k'][a] - Pi[k'][a] Pr[k][a])      (k, k': the rows of pair k)
// (tests/test_qf_four_products.py; float32 error not above the six-product form's, tools/qf_cog_check.py)
// -- the same numbers as transform, |.|^2, 2 x 2 binning and centre of gravity, to fp32 round-off.  Not usable with
// noise or when the image is wanted.
//
// On the matrix cores: lane (q, c) holds E[y = c][x = 4q + s], the A operand of E H' with the lane's constants
// h[s] = H'[4q + s][col(c)] as the B operand (8 instructions, Er and Ei); the results [y = 4q + r][col(c)] are the B
// operand of H'^T (E H') with the SAME four constants as the A operand (8 instructions), and P comes out as
// [row(4q + r)][col(c)].  The table orders the basis so that the two columns of a pair sit in lanes c and c ^ 2 and
// the two rows of a pair in registers r and r + 2 (aomarl_qf4_host.h: lane_column): the y moment is two packed
// products of the halves of the lane's own accumulators, the x moment one quad_perm read per register.
struct SpotQf { f32x4 h; f32x2 ky; float kx; };   // sys.qf_tab: h[s], (-2 t_{2q}, -2 t_{2q+1}), +-t of the lane's column

// The three moments of one sub-aperture, summed over the wave: returns z with  row 0 (lanes 0 .. 15): sum I,
// row 1: -sum (Y - 7.5) I, whole,  row 2: sum (X - 7.5) I / 2  (sign and the factors are folded into the table: see
// qf_slopes) -- every lane of a row holds the total.
// Round 6: 10 cross-lane instructions instead of 3 x 7 (tools/permlanebench.hip): gfx950's row swaps fold the four
// 16-lane rows of TWO registers into one (v_permlane32_swap: the upper half of the first operand against the lower
// half of the second -- [a_lo | b_lo] + [a_hi | b_hi]; v_permlane16_swap: the odd rows of the first against the even
// rows of the second), so that one register carries all three sums through the four in-row DPP steps.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float swap32_add(float a, float b) {
  const u32x2 t = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(t[0]) + __uint_as_float(t[1]);      // rows 0, 1: a (rows 0 + 2, 1 + 3); rows 2, 3: b
}
__device__ __forceinline__ float swap16_add(float a, float b) {
  const u32x2 t = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(t[0]) + __uint_as_float(t[1]);      // rows: a.0 + a.1, b.0 + b.1, a.2 + a.3, b.2 + b.3
}
// a[lane ^ 2] * b  and  acc += a[lane ^ 2] * b  (quad_perm [2,3,0,1]; every lane is active and has its partner)
__device__ __forceinline__ float dpp4e_mul(float a, float b) {
  float d;
  asm volatile("v_mul_f32_dpp %0, %1, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ void dpp4e_fmac(float &acc, float a, float b) {
  asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(acc) : "v"(a), "v"(b));
}
// What follows the matrix products, in three pieces that can be called one by one (the frame kernel's pair block
// puts the pieces of one tile between the matrix instructions of the other; spot_qf_moments runs them in a row):
// qf_products: the lane's terms of the three sums from P.  Hand-kept group: the CALLER opens it with the guard that
// covers the distance to the last matrix instruction that wrote Pr / Pi.
struct QfTerms { f32x2 p0, py; float px; };
__device__ __forceinline__ QfTerms qf_products(const SpotQf &K, const f32x4 Pr, const f32x4 Pi) {
  const f32x2 rl = pk_lo(Pr), rh = pk_hi(Pr), il = pk_lo(Pi), ih = pk_hi(Pi);
  // rows (r, r + 2) are a pair:  (Pi[0] Pr[2] - Pi[2] Pr[0],  Pi[1] Pr[3] - Pi[3] Pr[1]) . (-2 t_{2q}, -2 t_{2q+1});
  // columns (c, c ^ 2) are a pair: the lane's Pi against the partner's Pr, sign and t_k in the lane's constant.
  // The three chains take turns (a result is two instructions old when it is read), and the DPP products sit inside
  // the hand-kept group: one the compiler emits itself gets its own wait states for the matrix results on top of
  // the guard's.
  f32x2 p0 = pk_mul(rl, rl);
  f32x2 py = pk_mul(il, rh);
  float px = dpp4e_mul(Pr[0], Pi[0]);
  pk_acc_fma(p0, rh, rh);
  pk_acc_fnma(py, ih, rl);
  dpp4e_fmac(px, Pr[1], Pi[1]);
  pk_acc_fma(p0, il, il);
  py = pk_mul(py, K.ky);
  dpp4e_fmac(px, Pr[2], Pi[2]);
  pk_acc_fma(p0, ih, ih);
  dpp4e_fmac(px, Pr[3], Pi[3]);
  __builtin_amdgcn_sched_barrier(0);
  return QfTerms{p0, py, px};
}
// qf_fold_rows: the three sums of a lane into ONE register, one sum per 16-lane row
__device__ __forceinline__ float qf_fold_rows(const SpotQf &K, const QfTerms &m) {
  const float s0 = m.p0.x + m.p0.y, tx = m.px * K.kx, ty = m.py.x + m.py.y;
  // (the second operand of the second fold is a register that is dead by now: rows 2, 3 of that fold -- row 3 of z --
  // are never read, and a swap of ty with itself would need a copy first)
  return swap16_add(swap32_add(s0, tx), swap32_add(ty, m.p0.y));   // rows: s0, ty, tx, (unused)
}
// qf_fold_lanes: the row sums
__device__ __forceinline__ float qf_fold_lanes(float z) {
  z += dpp_f<0xB1>(z);      // quad_perm [1,0,3,2]
  z += dpp_f<0x4E>(z);      // quad_perm [2,3,0,1]
  z += dpp_f<0x141>(z);     // row_half_mirror
  z += dpp_f<0x140>(z);     // row_mirror -> every lane holds its 16-lane row sum
  return z;
}
__device__ __forceinline__ float spot_qf_moments(const SpotQf &K, const float (&er)[4], const float (&ei)[4], const f32x4 z4) {
  f32x4 Dr = z4, Di = z4;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    Dr = mfma16(er[s], K.h[s], Dr);              // (Er H')[y][a]
    Di = mfma16(ei[s], K.h[s], Di);              // (Ei H')[y][a]
  }
  f32x4 Pr = z4, Pi = z4;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    Pr = mfma16(K.h[r], Dr[r], Pr);              // (H'^T Er H')[b][a]
    Pi = mfma16(K.h[r], Di[r], Pi);              // (H'^T Ei H')[b][a]
  }
  PK_GUARD_MFMA();
  return qf_fold_lanes(qf_fold_rows(K, qf_products(K, Pr, Pi)));
}
// the two slopes of a sub-aperture from its moments (sum I, sum (X - 7.5) I / 2, -sum (Y - 7.5) I as
// spot_qf_moments leaves them: the factors and the sign are part of the table's constants)
__device__ __forceinline__ void qf_slopes(const DevSys &sys, float s0, float tx, float ty, float &sx, float &sy) {
  if (s0 > 0.f) {
    const float inv = __builtin_amdgcn_rcpf(s0);        // 1 ulp; slopes are compared at 1e-4"
    sx = (fmaf(tx, 2.f * inv, 7.5f) - sys.cog_offset) * sys.cog_scale;
    sy = (fmaf(-ty, inv, 7.5f) - sys.cog_offset) * sys.cog_scale;
  } else {
    sx = 0.f; sy = 0.f;
  }
}

// flux normalisation (+noise), COG on the binned quadrant values v[sy][sx][h]
template <bool NOISE, bool WRITE_CUBE>
__device__ __forceinline__ void spot_finish_v(const DevSys &sys, const DevState &st, int e, int i,
                                              int lane, const float (&v)[2][2][2], int do_cog,
                                              float flux_i) {
  const int q = lane >> 4, c = lane & 15;
  const bool owner = (c & 1) == 0;
  float tot = 0.f;
#pragma unroll
  for (int sy = 0; sy < 2; sy++)
#pragma unroll
    for (int sx = 0; sx < 2; sx++)
#pragma unroll
      for (int h = 0; h < 2; h++) tot += v[sy][sx][h];
  const int Xp = 8 + (c >> 1), Xm = 7 - (c >> 1);
  if (!NOISE && !WRITE_CUBE) {
    // only the slopes are wanted and nothing depends on the normalised pixel values: the COG is
    // invariant to the flux scale, so reduce (sum, sum x, sum y) of the raw image in ONE pass.  Every
    // binned pixel sits in both lanes of a pair (c, c ^ 1) with the same bits, so the sums over all
    // 64 lanes are exactly twice the image's: the factor drops out of the ratios, no lane is masked.
    const float A0 = (v[0][0][0] + v[0][0][1]) + (v[1][0][0] + v[1][0][1]);        // columns Xp
    const float A1 = (v[0][1][0] + v[0][1][1]) + (v[1][1][0] + v[1][1][1]);        // columns Xm
    float sx_ = (float)Xp * A0;
    sx_ = fmaf((float)Xm, A1, sx_);
    float sy_ = (float)(8 + 2 * q) * (v[0][0][0] + v[0][1][0]);
    sy_ = fmaf((float)(9 + 2 * q), v[0][0][1] + v[0][1][1], sy_);
    sy_ = fmaf((float)(7 - 2 * q), v[1][0][0] + v[1][1][0], sy_);
    sy_ = fmaf((float)(6 - 2 * q), v[1][0][1] + v[1][1][1], sy_);
    tot = wave_sum_last(A0 + A1);
    sx_ = wave_sum_last(sx_);
    sy_ = wave_sum_last(sy_);
    if (do_cog && lane == 63) {
      float *sl = st.slopes + (long long)e * sys.nslope;
      if (tot > 0.f) {
        const float inv = __builtin_amdgcn_rcpf(tot);       // 1 ulp; slopes are compared at 1e-4"
        sl[i] = (sx_ * inv - sys.cog_offset) * sys.cog_scale;
        sl[sys.nvalid + i] = (sy_ * inv - sys.cog_offset) * sys.cog_scale;
      } else {
        sl[i] = 0.f;
        sl[sys.nvalid + i] = 0.f;
      }
    }
    (void)flux_i;
    return;
  }
  // ---- total flux (each LR pixel is held by two lanes: count even lanes only)
  tot = wave_sum(owner ? tot : 0.f);
  const float g = tot > 0.f ? sys.nphot * flux_i / tot : 0.f;
  float s0 = 0.f, sx = 0.f, sy = 0.f;
  if (NOISE) {
    // the two lanes of a pair hold the same 8 pixels: lane parity h takes pixel h of each (ty, tx),
    // so every pixel gets its noise once and all 64 lanes work
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
      float *sl = st.slopes + (long long)e * sys.nslope;
      if (s0 != 0.f) {
        sl[i] = (sx / s0 - sys.cog_offset) * sys.cog_scale;
        sl[sys.nvalid + i] = (sy / s0 - sys.cog_offset) * sys.cog_scale;
      } else {
        sl[i] = 0.f;
        sl[sys.nvalid + i] = 0.f;
      }
    }
  }
}

template <bool NOISE, bool WRITE_CUBE>
__device__ __forceinline__ void spot_finish(const DevSys &sys, const DevState &st, int e, int i,
                                            int lane, const f32x4 (&Xr)[2][2],
                                            const f32x4 (&Xi)[2][2], int do_cog, float flux_i) {
  float v[2][2][2];
#pragma unroll
  for (int sy = 0; sy < 2; sy++)
#pragma unroll
    for (int sx = 0; sx < 2; sx++) spot_bin(Xr[sy][sx], Xi[sy][sx], v[sy][sx]);
  spot_finish_v<NOISE, WRITE_CUBE>(sys, st, e, i, lane, v, do_cog, flux_i);
}

// operands: br[s] / bi[s] = complex amplitude of pixel (y = c, x = 4q + s) of the tile
template <bool NOISE, bool WRITE_CUBE>
__device__ __forceinline__ void spot_core(const DevSys &sys, const DevState &st, int e, int i,
                                          int lane, const float (&Cc)[4], const float (&Ss)[4],
                                          const float (&br)[4], const float (&bi)[4], int do_cog,
                                          float flux_i, const f32x4 z4) {
  f32x4 Xr[2][2], Xi[2][2];           // [sy][sx], 0: +, 1: -
  spot_dft_f32(Cc, Ss, br, bi, z4, Xr, Xi);
  spot_finish<NOISE, WRITE_CUBE>(sys, st, e, i, lane, Xr, Xi, do_cog, flux_i);
}

template <bool NOISE, bool WRITE_CUBE>
__device__ __forceinline__ void spot_compute(const DevSys &sys, const DevState &st, int e, int i,
                                             int lane, int wv, const float (&Cc)[4],
                                             const float (&Ss)[4],
                                             float (*sAr)[16][17], float (*sAi)[16][17], int do_cog,
                                             float flux_i) {
  const int q = lane >> 4, c = lane & 15;
  float br[4], bi[4];
#pragma unroll
  for (int s = 0; s < 4; s++) { br[s] = sAr[wv][c][4 * q + s]; bi[s] = sAi[wv][c][4 * q + s]; }
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  spot_core<NOISE, WRITE_CUBE>(sys, st, e, i, lane, Cc, Ss, br, bi, do_cog, flux_i, z4);
}
