// aomarl_predictor_fn.h -- one frame of one series of the modal predictor (aomarl_predictor.hip): recursive least squares on
// the pseudo-open-loop mode x[t], stated on this simulator's delay line.  Plain C++ in one inline function, compiled by
// hipcc into k_pred_step and by the host compiler into predictor_host_check.cpp: the same text on both sides.
//
// With h[s] = (x[s], x[s-1], ..., x[s-N+1]) and (wa, wb, wc) the delay-line weights, the voltage of frame t is
// theta . phi for a constant theta, phi = wa h[t-1] + wb h[t-2] + wc h[t-3]; the filter learns the theta that nulls
//     eps = x[t] - theta . phi
// and commands c[t] = theta . h[t] with the theta AFTER the update (ao_marl_amd/predictive.py PredictorBank is the
// float64 statement).  The state of a series: theta[N], the upper triangle of P (row-major, N (N + 1) / 2), the N + 2
// past values x[t-1] ... x[t-N-2], J and J0.  Every index below is a compile-time constant once the loops are
// unrolled, so on the device the whole state stays in registers.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PR_HD __host__ __device__ __forceinline__
#else
#define PR_HD static inline
#endif

#define PR_MAXORDER 8
#define PR_TRI(N) ((N) * ((N) + 1) / 2)
#define PR_SLOTS(N) ((N) + PR_TRI(N) + (N) + 2 + 2)      // doubles per series: theta, P, past x, J, J0

// index of P[i][j], i <= j, in the row-major upper triangle
#define PR_IJ(N, i, j) ((i) * (N) - (i) * ((i) - 1) / 2 + ((j) - (i)))

template <int N> struct PredSeries {
  double th[N];
  double P[PR_TRI(N)];
  double xp[N + 2];          // xp[k] = x[t-1-k]
  double J, J0;
};

struct PredParams {
  double wa, wb, wc;
  double forget, iforget;    // iforget = 1 / forget
  double cap;                // order * p0: the largest trace P may have
};

// One frame.  count: this frame enters J and J0 (frames since the restart >= nskip); learn: theta and P are updated
// (learning is on and every regressor is a measured value: frames since the restart >= N + 2).  FORGET false: forget is
// 1 -- no factor on J, none on P, and no cap (the trace cannot grow).  Returns c[t] in double.
template <int N, bool FORGET> PR_HD double pred_step(PredSeries<N> &s, double x, const PredParams &p, bool count, bool learn) {
  double phi[N];
#pragma unroll
  for (int i = 0; i < N; i++) phi[i] = p.wa * s.xp[i] + p.wb * s.xp[i + 1] + p.wc * s.xp[i + 2];
  double pred = 0.0;
#pragma unroll
  for (int i = 0; i < N; i++) pred += s.th[i] * phi[i];
  const double eps = x - pred;
  if (count) {
    if (FORGET) { s.J = p.forget * s.J + eps * eps; s.J0 = p.forget * s.J0 + x * x; }
    else { s.J += eps * eps; s.J0 += x * x; }
  }
  if (learn) {
    double q[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < N; j++) a += s.P[i <= j ? PR_IJ(N, i, j) : PR_IJ(N, j, i)] * phi[j];
      q[i] = a;
    }
    double den = FORGET ? p.forget : 1.0;
#pragma unroll
    for (int i = 0; i < N; i++) den += phi[i] * q[i];
    const double inv = 1.0 / den, k = eps * inv;
#pragma unroll
    for (int i = 0; i < N; i++) s.th[i] += q[i] * k;
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) {
      const double qi = q[i] * inv;
#pragma unroll
      for (int j = i; j < N; j++) {
        double v = s.P[PR_IJ(N, i, j)] - qi * q[j];
        if (FORGET) v *= p.iforget;
        s.P[PR_IJ(N, i, j)] = v;
      }
      tr += s.P[PR_IJ(N, i, i)];
    }
    if (FORGET && tr > p.cap) {      // an unexcited series (an all-zero mode) must not blow P up under forget < 1
      const double f = p.cap / tr;
#pragma unroll
      for (int i = 0; i < PR_TRI(N); i++) s.P[i] *= f;
    }
  }
  double c = s.th[0] * x;
#pragma unroll
  for (int i = 1; i < N; i++) c += s.th[i] * s.xp[i - 1];
#pragma unroll
  for (int i = N + 1; i > 0; i--) s.xp[i] = s.xp[i - 1];
  s.xp[0] = x;
  return c;
}

// the start of a series: theta = (1, 0, ..., 0) -- the command is the last pseudo-open-loop mode --, P = p0 I
template <int N> PR_HD void pred_init(PredSeries<N> &s, double p0) {
#pragma unroll
  for (int i = 0; i < N; i++) s.th[i] = i == 0 ? 1.0 : 0.0;
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = i; j < N; j++) s.P[PR_IJ(N, i, j)] = i == j ? p0 : 0.0;
#pragma unroll
  for (int i = 0; i < N + 2; i++) s.xp[i] = 0.0;
  s.J = 0.0; s.J0 = 0.0;
}
