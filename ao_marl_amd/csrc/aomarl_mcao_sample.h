// aomarl_mcao_sample.h -- how a looking grid samples the plane of a mirror at altitude (aomarl_mcao.hip): bilinear_ring
// without the ring.  Zero outside the plane, the last line clamped; weights of zero give the floor cell's value exactly
// (1 v00 + 0 v01).  The operations are spelled out (every fused multiply-add written as one), so that the bits do not
// depend on the kernel the function is inlined into.
#pragma once

__device__ __forceinline__ float mcao_bilinear(const float *__restrict__ in, int N, float fx, float fy) {
  const int ix = (int)floorf(fx), iy = (int)floorf(fy);
  const float wx = fx - (float)ix, wy = fy - (float)iy;
  if (ix < 0 || iy < 0 || ix >= N || iy >= N) return 0.f;
  const int ix1 = ix + 1 < N ? ix + 1 : ix, iy1 = iy + 1 < N ? iy + 1 : iy;
  const float v00 = in[iy * N + ix], v01 = in[iy * N + ix1];
  const float v10 = in[iy1 * N + ix], v11 = in[iy1 * N + ix1];
  const float top = __builtin_fmaf(wx, v01, (1.f - wx) * v00), bot = __builtin_fmaf(wx, v11, (1.f - wx) * v10);
  return __builtin_fmaf(wy, bot, (1.f - wy) * top);
}
