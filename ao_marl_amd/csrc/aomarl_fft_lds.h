// aomarl_fft_lds.h -- radix-2 transforms over lines held in LDS, shared by the PSF reconstruction (aomarl_psfrec.hip)
// and the pyramid sensor (aomarl_pyr.hip).  Device code only.
// LDS layout: element i of line c lies at slot sw(i) * CW + c, sw(i) = i ^ (G - 1 where bit G of i is set), G = 32 / CW.
// A half wave (the conflict group of the 8-byte LDS accesses) handles G butterflies of CW lines; at stride s < G its
// elements are those of an aligned span of 2 G with bit s clear (or set), and the swizzle sends the two halves of that
// span to complementary slots: every stage reads and writes 32 distinct 8-byte slots of the 256-byte bank row.
#pragma once
#include <hip/hip_runtime.h>

template <int CW> __device__ __forceinline__ int pr_sw(int i) {
  constexpr int G = 32 / CW;
  return i ^ ((i & G) ? (G - 1) : 0);
}
__device__ __forceinline__ int pr_brev(int q, int logn) { return (int)(__brev((unsigned)q) >> (32 - logn)); }

// Decimation in frequency, natural order in, bit-reversed order out.
// x: CW lines of N = 2^logn points, laid out as above, written and synchronised by the caller.  Leaves X[brev(q)] of
// line c at slot pr_sw(q) * CW + c, synchronised.  tw[j] = exp(-2 pi i j / N), j < N / 2.
template <int CW>
__device__ __forceinline__ void pr_fft_lds(float2 *x, int logn, const float2 *__restrict__ tw, bool inv, int tid, int nthreads) {
  const int nbf = (1 << (logn - 1)) * CW;
  for (int ls = logn - 1; ls >= 0; ls--) {
    const int s = 1 << ls;
    for (int bf = tid; bf < nbf; bf += nthreads) {
      const int j = bf / CW, c = bf - j * CW;
      const int r = j & (s - 1), i = ((j >> ls) << (ls + 1)) + r;
      float2 w = tw[r << (logn - 1 - ls)];
      if (inv) w.y = -w.y;
      const int ia = pr_sw<CW>(i) * CW + c, ib = pr_sw<CW>(i + s) * CW + c;
      const float2 a = x[ia], b = x[ib];
      const float dx = a.x - b.x, dy = a.y - b.y;
      x[ia] = make_float2(a.x + b.x, a.y + b.y);
      x[ib] = make_float2(dx * w.x - dy * w.y, dx * w.y + dy * w.x);
    }
    __syncthreads();
  }
}

// Decimation in time, the network above run backwards: bit-reversed order in (X[brev(q)] of line c at slot
// pr_sw(q) * CW + c, as pr_fft_lds leaves it), natural order out, synchronised.  inv: the un-normalised inverse
// (conjugate twiddles), so that pr_fft_lds(inv = false) followed by pr_fft_dit_lds(inv = true) gives N x.
template <int CW>
__device__ __forceinline__ void pr_fft_dit_lds(float2 *x, int logn, const float2 *__restrict__ tw, bool inv, int tid, int nthreads) {
  const int nbf = (1 << (logn - 1)) * CW;
  for (int ls = 0; ls < logn; ls++) {
    const int s = 1 << ls;
    for (int bf = tid; bf < nbf; bf += nthreads) {
      const int j = bf / CW, c = bf - j * CW;
      const int r = j & (s - 1), i = ((j >> ls) << (ls + 1)) + r;
      float2 w = tw[r << (logn - 1 - ls)];
      if (inv) w.y = -w.y;
      const int ia = pr_sw<CW>(i) * CW + c, ib = pr_sw<CW>(i + s) * CW + c;
      const float2 a = x[ia], b = x[ib];
      const float bx = b.x * w.x - b.y * w.y, by = b.x * w.y + b.y * w.x;
      x[ia] = make_float2(a.x + bx, a.y + by);
      x[ib] = make_float2(a.x - bx, a.y - by);
    }
    __syncthreads();
  }
}
