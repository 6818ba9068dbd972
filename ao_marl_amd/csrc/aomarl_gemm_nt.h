// aomarl_gemm_nt.h -- the 64 x 64 GEMM kernels of the environment unit (included by aomarl_kernels.hip, after the
// split-fp16 helpers of aomarl_spot_dev.h): k_gemm_nt, k_gemm_nt_h, k_gemm_batched_gen, the split-K reduces, and launch_gemm_nt, the one
// host function every product of the AO loop goes through (its decisions: aomarl_gemm_plan_host.h).
#pragma once
#include "aomarl_gemm_plan_host.h"

// =============================================================================================
// fp32 GEMM  C[M][N] = alpha * A[M][K] . B[N][K]^T + beta * C     (both operands K-contiguous), ANY alignment:
// the fallback behind k_gemm_p (aomarl_gemm_p.h), which wants 16-byte aligned rows.  Element-wise loads,
// 256 threads = 4 waves in 2x2, block tile 64x64, one v_mfma_f32_32x32x2_f32 accumulator/wave.
// =============================================================================================
__global__ __launch_bounds__(256) void k_gemm_nt(int M, int N, int K, float alpha,
                                                 const float *__restrict__ A, int lda,
                                                 const float *__restrict__ B, int ldb, float beta,
                                                 float *__restrict__ C, int ldc, int kchunk,
                                                 float *__restrict__ P) {
  // blockIdx.z = K split: the block reduces k in [z*kchunk, min(K, (z+1)*kchunk)); with more than
  // one split the raw partial tile goes to P[z][M][N] and k_gemm_reduce finishes (deterministic)
  __shared__ float As[64][17];
  __shared__ float Bs[64][17];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int kb = blockIdx.z * kchunk, ke = min(K, kb + kchunk);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.f;
  const int lr = tid >> 2, lc = (tid & 3) * 4;
  const int gm = m0 + lr, gn = n0 + lr;
  const float *pa = A + (long long)gm * lda;
  const float *pb = B + (long long)gn * ldb;
  for (int k0 = kb; k0 < ke; k0 += 16) {
    float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f};
    const int gk = k0 + lc;
    if (gm < M) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (gk + j < ke) va[j] = pa[gk + j];
    }
    if (gn < N) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (gk + j < ke) vb[j] = pb[gk + j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      As[lr][lc + j] = va[j];
      Bs[lr][lc + j] = vb[j];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
      float a = As[wm * 32 + (lane & 31)][2 * ks + (lane >> 5)];
      float b = Bs[wn * 32 + (lane & 31)][2 * ks + (lane >> 5)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const int col = n0 + wn * 32 + (lane & 31);
  const bool split = gridDim.z > 1;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < M && col < N) {
      if (split) {
        P[((long long)blockIdx.z * M + row) * N + col] = acc[r];
      } else {
        float *c = C + (long long)row * ldc + col;
        float v = alpha * acc[r];
        if (beta != 0.f) v += beta * (*c);
        *c = v;
      }
    }
  }
}


// LDS row stride of k_gemm_batched_gen's 64 x 32 tiles (floats): the 16 lanes of a 128-bit read pass hit 64 distinct banks
#define G2_LD 36

// ---------------------------------------------------------------------------------------------
// The same GEMM on the f16 matrix pipe with SPLIT operands: every fp32 value v is carried as
// hi = f16(v), lo = f16(v - hi), both rounded to nearest (23 significant bits, unbiased) and a product
// as hi.hi + lo.hi + hi.lo with fp32 accumulation (lo.lo, <= 2^-24 of a product, dropped): three v_mfma_f32_32x32x16_f16 of 32 cycles
// each per 16 k against sixteen 64-cycle v_mfma_f32_32x32x2_f32 (fp32 matrix instructions run at the
// packed-fp32 vector rate on this chip) -- 10x less matrix-pipe time; what is left is the splitting
// (2 vector instructions per element as it is staged into LDS) and the LDS traffic.
// Operands stay fp32 in memory, same interface as k_gemm_nt plus a power-of-two scale per operand
// (sa, sb; applied as the values are staged, undone through alpha): the scaled values must stay
// below 65504 (they saturate above) and lose low bits of `lo` below 6e-5 (absolute error <= 3e-8
// of the scaled value).  gemm_scale() picks the scale of a static matrix from its largest entry.
// LDS: hi and lo planes of the A and B tiles as f16, [row][32 k] with a row stride of 40 halfs (a
// 16-lane pass of a 128-bit read -- 8 k of one row per lane -- covers the 64 banks exactly once).
// ---------------------------------------------------------------------------------------------
#define GH_LD 40
typedef _Float16 hx4 __attribute__((ext_vector_type(4)));
// round-to-nearest-even pair (v_cvt_pk_f16_f32): unbiased, unlike the truncating v_cvt_pkrtz -- a GEMM
// adds thousands of products, a truncation bias would add up linearly
typedef float fx2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ hx2 cvt_rn2(float a, float b) {
  const fx2 v = {a, b};
  return __builtin_convertvector(v, hx2);
}
__device__ __forceinline__ void gh_split(float4 v, const float scale, hx4 &hi, hx4 &lo, float &amax) {
  // power of two: exact; clamped to the f16 range (a value beyond it -- a centroid whose total flux
  // came out ~0 -- saturates instead of turning into inf - inf = NaN).  amax: largest scaled magnitude this
  // thread staged; the kernel counts the threads that saw one above the range (aomarl_gemm_saturated)
  v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
  amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  v.x = __builtin_amdgcn_fmed3f(v.x, -65504.f, 65504.f); v.y = __builtin_amdgcn_fmed3f(v.y, -65504.f, 65504.f);
  v.z = __builtin_amdgcn_fmed3f(v.z, -65504.f, 65504.f); v.w = __builtin_amdgcn_fmed3f(v.w, -65504.f, 65504.f);
  const hx2 h01 = cvt_rn2(v.x, v.y), h23 = cvt_rn2(v.z, v.w);
  const hx2 l01 = cvt_rn2(sub_lo(h01, v.x), sub_hi(h01, v.y));   // |v - hi| <= 2^-12 |v|, lo keeps 11 bits of it
  const hx2 l23 = cvt_rn2(sub_lo(h23, v.z), sub_hi(h23, v.w));
  hi = hx4{h01[0], h01[1], h23[0], h23[1]};
  lo = hx4{l01[0], l01[1], l23[0], l23[1]};
}

// Three k-tiles of global loads are in flight per thread (register stages, loop unrolled by three):
// with the 10-20 k-tiles a split-K block walks, one tile ahead left the loop waiting for L2 / HBM on
// every iteration.  The loop body has NO branch around a load and no select on a load's result: the
// loads are unconditional (addresses clamped into the row; a tile past the end of the chunk is masked
// to zero as it is staged into LDS, so the loop simply runs whole groups of three tiles) -- with
// either, the compiler waits for the data where it is loaded and the three stages collapse into one
// (3 000 lines of branchy ISA and 20 us per call; measured).  Scheduling barriers keep the loads where
// they are written.  Callers make the chunk a multiple of 96 so that only the last chunk has padding.
__device__ __forceinline__ void gh_mainloop(const float *__restrict__ A, int lda,
                                            const float *__restrict__ B, int ldb, int M, int N,
                                            int m0, int n0, int kb, int ke, _Float16 *S, f32x16 &acc,
                                            const float sa, const float sb, float &amax) {
  // S: [2 buffers][4 planes: A hi, A lo, B hi, B lo][64 rows][GH_LD]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int lr = tid >> 3, lc = (tid & 7) * 4;
  const float *pa0 = A + (long long)min(m0 + lr, M - 1) * lda;
  const float *pa1 = A + (long long)min(m0 + lr + 32, M - 1) * lda;
  const float *pb0 = B + (long long)min(n0 + lr, N - 1) * ldb;
  const float *pb1 = B + (long long)min(n0 + lr + 32, N - 1) * ldb;
  const int klast = (ke - 1) & ~3;               // last 16-byte group that holds a valid element (lda, ldb >= its end)
  constexpr int ST = 3;                          // register stages
  float4 ra0[ST], ra1[ST], rb0[ST], rb1[ST];
  auto gload = [&](int k0, int st) {             // st: compile-time after unrolling
    const int k = min(k0 + lc, klast);
    ra0[st] = *reinterpret_cast<const float4 *>(pa0 + k); ra1[st] = *reinterpret_cast<const float4 *>(pa1 + k);
    rb0[st] = *reinterpret_cast<const float4 *>(pb0 + k); rb1[st] = *reinterpret_cast<const float4 *>(pb1 + k);
  };
  constexpr int PL = 64 * GH_LD;                 // halfs per plane
  auto lstore = [&](int buf, int st, int k0) {
    _Float16 *s = S + buf * 4 * PL;
    float4 a0 = ra0[st], a1 = ra1[st], b0 = rb0[st], b1 = rb1[st];
    if (k0 + 32 > ke) {                          // wave-uniform: the tile crosses the end of the chunk
      const int k = k0 + lc;
      const bool m0_ = k < ke, m1_ = k + 1 < ke, m2_ = k + 2 < ke, m3_ = k + 3 < ke;
      auto msk = [&](float4 &v) { v.x = m0_ ? v.x : 0.f; v.y = m1_ ? v.y : 0.f; v.z = m2_ ? v.z : 0.f; v.w = m3_ ? v.w : 0.f; };
      msk(a0); msk(a1); msk(b0); msk(b1);
    }
    hx4 h, l;
    gh_split(a0, sa, h, l, amax);
    *reinterpret_cast<hx4 *>(s + lr * GH_LD + lc) = h; *reinterpret_cast<hx4 *>(s + PL + lr * GH_LD + lc) = l;
    gh_split(a1, sa, h, l, amax);
    *reinterpret_cast<hx4 *>(s + (lr + 32) * GH_LD + lc) = h; *reinterpret_cast<hx4 *>(s + PL + (lr + 32) * GH_LD + lc) = l;
    gh_split(b0, sb, h, l, amax);
    *reinterpret_cast<hx4 *>(s + 2 * PL + lr * GH_LD + lc) = h; *reinterpret_cast<hx4 *>(s + 3 * PL + lr * GH_LD + lc) = l;
    gh_split(b1, sb, h, l, amax);
    *reinterpret_cast<hx4 *>(s + 2 * PL + (lr + 32) * GH_LD + lc) = h; *reinterpret_cast<hx4 *>(s + 3 * PL + (lr + 32) * GH_LD + lc) = l;
  };
  // operand of lane l for k-chunk c (16 k): row (l & 31) of the wave's 32, k = 16 c + 8 (l >> 5) .. + 7
  const int ro = (lane & 31) * GH_LD + 8 * (lane >> 5);
#pragma unroll
  for (int st = 0; st < ST; st++) gload(kb + 32 * st, st);
  __builtin_amdgcn_sched_barrier(0);
  lstore(0, 0, kb);
  gload(kb + 32 * ST, 0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += 32 * ST) {
#pragma unroll
    for (int u = 0; u < ST; u++) {
      const int kc = k0 + 32 * u;                // the tile in LDS buffer `buf` (all zeros past the end)
      // tile kc + 32 sits in register stage (u + 1) % ST: split it into the other LDS buffer, then
      // reuse that stage for tile kc + 32 (ST + 1); only then the matrix instructions on this tile
      lstore(buf ^ 1, (u + 1) % ST, kc + 32);
      gload(kc + 32 * (ST + 1), (u + 1) % ST);
      __builtin_amdgcn_sched_barrier(0);
      const _Float16 *s = S + buf * 4 * PL;
      const _Float16 *ah = s + wm * 32 * GH_LD + ro, *al = ah + PL;
      const _Float16 *bh = s + 2 * PL + wn * 32 * GH_LD + ro, *bl = bh + PL;
#pragma unroll
      for (int cch = 0; cch < 2; cch++) {
        const hx8 Ah = *reinterpret_cast<const hx8 *>(ah + 16 * cch), Al = *reinterpret_cast<const hx8 *>(al + 16 * cch);
        const hx8 Bh = *reinterpret_cast<const hx8 *>(bh + 16 * cch), Bl = *reinterpret_cast<const hx8 *>(bl + 16 * cch);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl, acc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
      buf ^= 1;
    }
  }
}

__global__ __launch_bounds__(256) void k_gemm_nt_h(int M, int N, int K, float alpha,
                                                   const float *__restrict__ A, int lda,
                                                   const float *__restrict__ B, int ldb, float beta,
                                                   float *__restrict__ C, int ldc, int kchunk,
                                                   float *__restrict__ P, float sa, float sb, int xcd,
                                                   unsigned *__restrict__ sat) {
  __shared__ __attribute__((aligned(16))) _Float16 S[2 * 4 * 64 * GH_LD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wm = wv >> 1, wn = wv & 1;
  // Workgroups go to the 8 XCDs round-robin in launch order, each XCD with its own 4 MB L2.  With the
  // plain (x, y, z) order every XCD sees tiles of every k-chunk, i.e. streams BOTH operands whole
  // (5 + 6 MB for an extrusion round) through its L2; remapped, XCD q owns a contiguous range of the
  // z-major order -- about one k-chunk, 1.6 MB of operands.  Worth 2.5 % of a reset (45.8 -> 44.6 ms),
  // no more: the kernel is not bound by where its operands come from (the GEMM notes).
  int bxi = blockIdx.x, byi = blockIdx.y, bzi = blockIdx.z;
  if (xcd) {
    const int T = gridDim.x * gridDim.y * gridDim.z;
    const int L = bxi + gridDim.x * (byi + gridDim.y * bzi);
    const int q = L & 7, i = L >> 3;
    const int lg = q * (T >> 3) + min(q, T & 7) + i;
    const int xy = gridDim.x * gridDim.y;
    bzi = lg / xy;
    const int r = lg - bzi * xy;
    byi = r / gridDim.x; bxi = r - byi * gridDim.x;
  }
  const int m0 = byi * 64, n0 = bxi * 64;
  const int kb = bzi * kchunk, ke = min(K, kb + kchunk);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.f;
  float amax = 0.f;
  gh_mainloop(A, lda, B, ldb, M, N, m0, n0, kb, ke, S, acc, sa, sb, amax);
  if (amax > 65504.f) atomicAdd(sat, 1u);        // a scaled operand left the fp16 range and was clipped (rare: one atomic per such thread)
  const int col = n0 + wn * 32 + (lane & 31);
  const bool split = gridDim.z > 1;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < M && col < N) {
      if (split) {
        P[((long long)bzi * M + row) * N + col] = acc[r];
      } else {
        float *c = C + (long long)row * ldc + col;
        float v = alpha * acc[r];
        if (beta != 0.f) v += beta * (*c);
        *c = v;
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// General batched GEMM for the SAC networks' forward AND backward passes:
//     C[b] = act( opA(A[b]) . opB(B[b]) + bias[b] ) (+ C[b] when accumulate)
// opA(A) is M x K, opB(B) is K x N.  TA = false: A stored [M][K] (K contiguous); TA = true: A stored
// [K][M].  TB = false: B stored [N][K] (the "NT" form above); TB = true: B stored [K][N].
// The three products of a linear layer y = x W (W stored [in][out]) are
//     forward  y  = x . W        TA = 0, TB = 1        backward dx = dy . W^T     TA = 0, TB = 0
//     weights  dW = x^T . dy     TA = 1, TB = 1
// 64 x 64 tile, LDS rows of 36 floats, one 32x32x2 accumulator per wave; a k-strided operand is read with 128-bit loads
// along its contiguous (row) direction and transposed on the way into LDS.
// ---------------------------------------------------------------------------------------------
template <bool T>
__device__ __forceinline__ void gg_load(const float *__restrict__ P, int ld, int rows, int r0, int k0,
                                        int ke, int tid, float (&v)[8], bool vec) {
  // this thread's 8 elements of the 64 (rows) x 32 (k) tile starting at (r0, k0)
  if (!T) {
    const int lr = tid >> 3, lc = (tid & 7) * 4;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int r = min(r0 + lr + 32 * h, rows - 1);
      const float *p = P + (long long)r * ld;
      const int k = k0 + lc;
      if (k + 3 < ke && vec) {
        const float4 t = *reinterpret_cast<const float4 *>(p + k);
        v[4 * h] = t.x; v[4 * h + 1] = t.y; v[4 * h + 2] = t.z; v[4 * h + 3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[4 * h + j] = (k + j < ke) ? p[k + j] : 0.f;
      }
    }
  } else {
    const int kk = tid >> 4, r4 = (tid & 15) * 4;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = k0 + kk + 16 * h;
      const float *p = P + (long long)k * ld;
      if (k < ke) {
        if (r0 + r4 + 3 < rows && vec) {
          const float4 t = *reinterpret_cast<const float4 *>(p + r0 + r4);
          v[4 * h] = t.x; v[4 * h + 1] = t.y; v[4 * h + 2] = t.z; v[4 * h + 3] = t.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) v[4 * h + j] = p[min(r0 + r4 + j, rows - 1)];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[4 * h + j] = 0.f;
      }
    }
  }
}

template <bool T>
__device__ __forceinline__ void gg_store(float *S, int tid, const float (&v)[8]) {
  if (!T) {
    const int lr = tid >> 3, lc = (tid & 7) * 4;
#pragma unroll
    for (int h = 0; h < 2; h++)
      *reinterpret_cast<float4 *>(S + (lr + 32 * h) * G2_LD + lc) = make_float4(v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]);
  } else {
    const int kk = tid >> 4, r4 = (tid & 15) * 4;
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int j = 0; j < 4; j++) S[(r4 + j) * G2_LD + kk + 16 * h] = v[4 * h + j];
  }
}

// G k-groups of 4 waves share one 64 x 64 output tile: group g runs the K slabs g, g + G, ... through
// its own double-buffered LDS stage, so G slabs are in flight per block (these products are small --
// 224 tiles for the SAC layers -- and with one wave per SIMD every slab paid the full L2 / MALL
// latency); the partial tiles are summed through LDS in a fixed order.
template <bool TA, bool TB, int G>
__global__ __launch_bounds__(256 * G) void k_gemm_batched_gen(int M, int N, int K,
                                                              const float *__restrict__ A, int lda, long long sA,
                                                              const float *__restrict__ B, int ldb, long long sB,
                                                              const float *__restrict__ bias, long long sBias,
                                                              float *__restrict__ C, int ldc, long long sC,
                                                              int relu, int accumulate, int vecA, int vecB,
                                                              const float *__restrict__ mask, int ldm, long long sM,
                                                              int tn, int tm, int ntile) {
  // mask (the layer's forward output, for the ReLU backward): C = acc where mask > 0, else 0
  extern __shared__ __attribute__((aligned(16))) float gsm[];
  // XCD-aware tile order: workgroups go round-robin over the 8 XCDs (each with its own L2), so
  // workgroup L runs tile (L % 8) * per + L / 8: the tiles of one matrix -- which share A rows and
  // B columns -- land on one XCD and fetch them into its L2 once instead of once per XCD.
  const int per = gridDim.x >> 3;
  const int w = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (w >= ntile) return;
  const int bz = w / (tn * tm), wt = w - bz * (tn * tm);
  const int grp = threadIdx.x >> 8, tid = threadIdx.x & 255;
  float *As = gsm + grp * (4 * 64 * G2_LD), *Bs = As + 2 * 64 * G2_LD;
  const int lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int m0 = (wt / tn) * 64, n0 = (wt % tn) * 64;
  A += (long long)bz * sA; B += (long long)bz * sB; C += (long long)bz * sC;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.f;
  const int nslab = (K + 31) / 32, nloop = (nslab + G - 1) / G;      // block-uniform trip count
  float va[8], vb[8];
  if (grp < nslab) {
    gg_load<TA>(A, lda, M, m0, grp * 32, K, tid, va, vecA);
    gg_load<TB>(B, ldb, N, n0, grp * 32, K, tid, vb, vecB);
    gg_store<TA>(As, tid, va);
    gg_store<TB>(Bs, tid, vb);
  }
  __syncthreads();
  const int ro = (lane & 31) * G2_LD + 16 * (lane >> 5);
  int buf = 0;
  for (int it = 0; it < nloop; it++, buf ^= 1) {
    const int slab = it * G + grp;
    const bool live = slab < nslab, more = slab + G < nslab;
    if (more) {
      gg_load<TA>(A, lda, M, m0, (slab + G) * 32, K, tid, va, vecA);
      gg_load<TB>(B, ldb, N, n0, (slab + G) * 32, K, tid, vb, vecB);
    }
    if (live) {
      const float *as = As + buf * 64 * G2_LD + wm * 32 * G2_LD + ro;
      const float *bs = Bs + buf * 64 * G2_LD + wn * 32 * G2_LD + ro;
      float4 a4[4], b4[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        a4[j] = *reinterpret_cast<const float4 *>(as + 4 * j);
        b4[j] = *reinterpret_cast<const float4 *>(bs + 4 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j].x, b4[j].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j].y, b4[j].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j].z, b4[j].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j].w, b4[j].w, acc, 0, 0, 0);
      }
    }
    if (more) {
      gg_store<TA>(As + (buf ^ 1) * 64 * G2_LD, tid, va);
      gg_store<TB>(Bs + (buf ^ 1) * 64 * G2_LD, tid, vb);
    }
    __syncthreads();
  }
  if (G > 1) {
    // partial tiles of groups 1 .. G-1 -> LDS [g-1][r][256 threads]; group 0 adds them in order
    if (grp > 0) {
      float *red = gsm + (grp - 1) * (16 * 256);
#pragma unroll
      for (int r = 0; r < 16; r++) red[r * 256 + tid] = acc[r];
    }
    __syncthreads();
    if (grp > 0) return;
#pragma unroll
    for (int g = 1; g < G; g++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] += gsm[(g - 1) * (16 * 256) + r * 256 + tid];
  }
  const int col = n0 + wn * 32 + (lane & 31);
  const float bv = (bias && col < N) ? bias[(long long)bz * sBias + col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < M && col < N) {
      float *c = C + (long long)row * ldc + col;
      float v = acc[r] + bv;
      if (accumulate) v += *c;
      if (relu) v = fmaxf(v, 0.f);
      if (mask && !(mask[(long long)bz * sM + (long long)row * ldm + col] > 0.f)) v = 0.f;
      *c = v;
    }
  }
}

__global__ void k_gemm_reduce(int M, int N, int nsplit, float alpha, const float *__restrict__ P,
                              float beta, float *__restrict__ C, int ldc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)M * N) return;
  const int row = (int)(i / N), col = (int)(i - (long long)row * N);
  const float s = slab_sum<4>(nsplit, [&](int z) { return P[(long long)z * M * N + i]; });
  float *c = C + (long long)row * ldc + col;
  float v = alpha * s;
  if (beta != 0.f) v += beta * (*c);
  *c = v;
}

// split-K reduce with the consumer's element-wise step folded in (saves that launch):
//   mode 1: C = err, com += gain * err                                (Rtc.do_control)
//   mode 2: C = modes, modes[m] += action[j] * freedom[m] for the action modes  (rl_control)
struct GemmEpi {
  int mode;
  float *com; int ldcom; float gain;
  const float *gain_row;               // mode 1: per-row (per-environment) integrator gains, or null
  const float *action; int nact; const int32_t *amode_inv; const float *freedom;
};

__global__ void k_gemm_reduce_epi(int M, int N, int nsplit, float alpha, const float *__restrict__ P,
                                  float beta, float *__restrict__ C, int ldc, GemmEpi ep) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)M * N) return;
  const int row = (int)(i / N), col = (int)(i - (long long)row * N);
  const float s = slab_sum<4>(nsplit, [&](int z) { return P[(long long)z * M * N + i]; });
  float *c = C + (long long)row * ldc + col;
  float v = alpha * s;
  if (beta != 0.f) v += beta * (*c);
  if (ep.mode == 1) {
    ep.com[(long long)row * ep.ldcom + col] += (ep.gain_row ? ep.gain_row[row] : ep.gain) * v;
  } else if (ep.mode == 2) {
    const int j = ep.amode_inv[col];
    if (j >= 0) v += ep.action[(long long)row * ep.nact + j] * ep.freedom[col];
  }
  *c = v;
}

// power-of-two scale that brings the largest magnitude of a matrix to ~4096 (f16: 11 bits, max 65504)
static float gemm_scale(const float *h, size_t n) {
  float m = 0.f;
  for (size_t i = 0; i < n; i++) m = std::max(m, fabsf(h[i]));
  if (!(m > 0.f) || !std::isfinite(m)) return 1.f;
  int e = (int)floorf(log2f(4096.f / m));
  e = std::max(-10, std::min(24, e));
  return ldexpf(1.f, e);
}
// the process-wide options of launch_gemm_nt ("gemm_split_f16" follows aomarl_set_precision; see the arithmetic
// note in aomarl_kernels.hip)
static GemmOptions g_gemm = {/* xcd */ 1, /* target_blocks */ 0, /* split_f16 */ false};
static int g_gemm_kgroups = 0;       // batched general GEMM: 0 = by heuristic; 1 / 2 / 4 forced
// Retired after their A/B runs (profiles/r01g_*): the un-pipelined and the pipelined aligned 64 x 64 kernels (k_gemm_p
// took their place) and an in-kernel split-K reduction through ticket counters (4x slower: every block pays an
// L2 write-back for its __threadfence).  k_gemm_nt stays as the fallback for operands that are not 16-byte aligned.

// Threads of k_gemm_nt_h launches that staged an operand beyond the fp16 range (clipped to +-65504): one
// counter per device, read and cleared by aomarl_gemm_saturated.  The internal call sites scale their
// operands with margins of 10^2 .. 10^4 over what a closed loop produces (stencil differences x 2^8 up to
// 255 um, modes x 2^4 up to 4094, slopes x 1); a diverging policy or a runaway loop can leave them.
static unsigned *g_gemm_sat[64] = {nullptr};
static unsigned *gemm_sat_counter() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!g_gemm_sat[dev]) {
    void *p = nullptr;
    if (hipMalloc(&p, sizeof(unsigned)) != hipSuccess || hipMemset(p, 0, sizeof(unsigned)) != hipSuccess) return nullptr;
    g_gemm_sat[dev] = (unsigned *)p;
  }
  return g_gemm_sat[dev];
}

// aomarl_gemm_nt_probe (tests only): the kernel, tile, k split and block numbering to take instead of the library's
// own, and a report of what was launched.  A refusal leaves error set and launches nothing.
struct GemmForce {
  GemmForceIn in;
  const char *error;     // out: null, or what was refused
  int r_kernel, r_wm, r_wn, r_nz, r_kchunk;       // out: what was launched
  GemmPCfg pick;         // out: GemmPlan::pick
};

struct GemmArgs {
  int M, N, K;
  float alpha;
  const float *A; int lda;
  const float *B; int ldb;
  float beta;
  float *C; int ldc;
  hipStream_t s;
  float *ws = nullptr; size_t ws_floats = 0;     // optional split-K workspace (null: never split)
  const GemmEpi *epi = nullptr;                  // applied by the split-K reduce when there is one (GemmDone::epi_done), else left to the caller
  bool slabs_only = false;                       // a split product launches NO reduce: the caller's next kernel sums the partial tiles ws[z][M][N] itself
  bool fast = false; float sa = 1.f, sb = 1.f;   // the split-f16 kernel may be used, with these power-of-two scales (GemmQuery::fast)
  int min_chunk = 128;                           // GemmQuery::min_chunk
  int pick_M = 0;                                // GemmQuery::pick_M
  GemmForce *force = nullptr;
  GemmArgs(int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb, float beta, float *C,
           int ldc, hipStream_t s)
      : M(M), N(N), K(K), alpha(alpha), A(A), lda(lda), B(B), ldb(ldb), beta(beta), C(C), ldc(ldc), s(s) {}
};
struct GemmDone {
  bool epi_done;         // the epilogue ran in the split-K reduce
  int slabs;             // slabs_only: the partial tiles the caller has to sum (0: C is final)
  float slab_alpha;      // ... and the factor to apply to their sum
};

static GemmDone launch_gemm_nt(const GemmArgs &a, const GemmOptions &opt = g_gemm) {
  const int M = a.M, N = a.N, K = a.K;
  GemmForce *force = a.force;
  GemmDone done = {false, 0, a.alpha};
  const bool al = (a.lda % 4 == 0) && (a.ldb % 4 == 0) && (((uintptr_t)a.A & 15) == 0) && (((uintptr_t)a.B & 15) == 0);
  const GemmQuery q = {M, N, K, al, a.ws ? a.ws_floats : 0, a.fast, a.min_chunk, a.pick_M};
  GemmPlan p = gemm_plan(q, opt, force ? &force->in : nullptr);
  if (p.kernel == GEMM_NONE && !p.error) return done;        // an empty product
  if (force) {
    force->error = p.error;
    force->r_kernel = force->r_wm = force->r_wn = force->r_nz = force->r_kchunk = 0;
    force->pick = p.pick;
  }
  if (p.error) return done;
  float alpha = a.alpha;
  int nz = p.p.nz;
  if (p.kernel == GEMM_P) {
    if (p.p.wm > 0 && gemm_p_launch(p.p, M, N, K, alpha, a.A, a.lda, a.B, a.ldb, a.beta, a.C, a.ldc, a.ws, p.xcd, a.s)) {
      g_arith[AR_GEMM_F32]++;
      if (force) { force->r_kernel = 1; force->r_wm = p.p.wm; force->r_wn = p.p.wn; force->r_nz = nz; force->r_kchunk = p.p.kchunk; }
    } else {
      if (force && (force->in.kernel == 1 || force->in.wm)) { force->error = "kernel (k_gemm_p could not be launched)"; return done; }
      gemm_plan_fallback(q, opt, force ? &force->in : nullptr, &p);
      if (p.error) { if (force) force->error = p.error; return done; }
    }
  }
  if (p.kernel != GEMM_P) {
    nz = p.nz;
    const dim3 grid((N + 63) / 64, (M + 63) / 64, nz);
    unsigned *sat = p.kernel == GEMM_NT_H ? gemm_sat_counter() : nullptr;
    if (force && force->in.kernel == 3 && !sat) { force->error = "kernel (no saturation counter for k_gemm_nt_h)"; return done; }
    if (force) { force->r_kernel = sat ? 3 : 2; force->r_wm = force->r_wn = 2; force->r_nz = nz; force->r_kchunk = p.kchunk; }
    if (sat) {
      alpha /= (a.sa * a.sb);                      // also what the split-K reduce below applies
      done.slab_alpha = alpha;
      hipLaunchKernelGGL(k_gemm_nt_h, grid, dim3(256), 0, a.s, M, N, K, alpha, a.A, a.lda, a.B, a.ldb, a.beta, a.C,
                         a.ldc, p.kchunk, a.ws, a.sa, a.sb, p.xcd, sat);
      g_arith[AR_GEMM_SPLIT]++;
    } else {
      hipLaunchKernelGGL(k_gemm_nt, grid, dim3(256), 0, a.s, M, N, K, alpha, a.A, a.lda, a.B, a.ldb, a.beta, a.C,
                         a.ldc, p.kchunk, a.ws);
      g_arith[AR_GEMM_F32]++;
    }
  }
  if (nz > 1) {
    const dim3 rgrid((unsigned)(((long long)M * N + 255) / 256));
    if (a.slabs_only) {
      done.slabs = nz;
    } else if (a.epi) {
      hipLaunchKernelGGL(k_gemm_reduce_epi, rgrid, dim3(256), 0, a.s, M, N, nz, alpha, a.ws, a.beta, a.C, a.ldc, *a.epi);
      done.epi_done = true;
    } else {
      hipLaunchKernelGGL(k_gemm_reduce, rgrid, dim3(256), 0, a.s, M, N, nz, alpha, a.ws, a.beta, a.C, a.ldc);
    }
  }
  return done;
}
