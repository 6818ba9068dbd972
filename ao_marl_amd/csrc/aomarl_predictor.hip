// aomarl_predictor.hip -- modal predictive control: one recursive-least-squares predictor per (environment, Btt mode) on
// the pseudo-open-loop modes, stated on this simulator's delay line.  gfx950 only.
//
// Upstream has no predictive controller in the reference tree; this is the published method (recursive least squares on
// pseudo-open-loop telemetry) on THIS simulator's loop model (aomarl_modopti_host.h): the voltage of frame t is
// wa c[t-1] + wb c[t-2] + wc c[t-3], so a command c[s] = theta . h[s], h[s] = (x[s], ..., x[s-N+1]), leaves the residual
//     eps[t] = x[t] - theta . (wa h[t-1] + wb h[t-2] + wc h[t-3])
// and the filter learns the theta that nulls it (aomarl_predictor_fn.h: the update, shared with the host check;
// ao_marl_amd/predictive.py PredictorBank: the float64 statement).
//   state [PR_SLOTS(N)][nenv nmodes] double, slot-major: theta[N], the upper triangle of P, the N + 2 past values, J, J0
//         -- the 64 lanes of a wave read and write 512 contiguous bytes per slot
//   k_pred_step<N, LEARN, FORGET>  one lane per series; the order is a template parameter so that every index into the
//         state is a compile-time constant and the state lives in registers for all the frames of a call (a run-time
//         index would put it into scratch).  No LDS, no atomics, no cross-lane operation: the same inputs, the same
//         bits, however the frames are split over calls.
//   k_pred_get  the state unpacked into [series][...] arrays, P as the full symmetric matrix
#include "aomarl_host.h"
#include "aomarl_predictor_host.h"
#include <vector>
#include <string.h>

#define PR_BLOCK 64

template <int N, bool LEARN, bool FORGET>
__global__ __launch_bounds__(PR_BLOCK) void k_pred_step(const float *__restrict__ x, long long stride, int nframes, int nseries,
                                                        int nm, double *__restrict__ state, float *__restrict__ c_out,
                                                        long long c_stride, int c_ld, float *__restrict__ last_x,
                                                        float *__restrict__ last_c, PredParams p, long long f0, long long nskip) {
  const int S = blockIdx.x * PR_BLOCK + threadIdx.x;
  if (S >= nseries) return;
  const size_t ns = (size_t)nseries;
  double *st = state + S;
  PredSeries<N> s;
  int k = 0;
#pragma unroll
  for (int i = 0; i < N; i++) s.th[i] = st[(size_t)(k++) * ns];
#pragma unroll
  for (int i = 0; i < PR_TRI(N); i++, k++) s.P[i] = LEARN ? st[(size_t)k * ns] : 0.0;      // (frozen: P is neither read nor written)
#pragma unroll
  for (int i = 0; i < N + 2; i++) s.xp[i] = st[(size_t)(k++) * ns];
  s.J = st[(size_t)(k++) * ns];
  s.J0 = st[(size_t)(k++) * ns];
  const long long co = c_ld == nm ? (long long)S : (long long)(S / nm) * c_ld + S % nm;
  float xf = 0.f, cf = 0.f;
  for (int t = 0; t < nframes; t++) {
    xf = x[(long long)t * stride + S];
    const long long f = f0 + t;
    cf = (float)pred_step<N, FORGET>(s, (double)xf, p, f >= nskip, LEARN && f >= N + 2);
    if (c_out) c_out[(long long)t * c_stride + co] = cf;
  }
  if (last_x) last_x[S] = xf;
  last_c[S] = cf;
  k = 0;
#pragma unroll
  for (int i = 0; i < N; i++) st[(size_t)(k++) * ns] = s.th[i];
#pragma unroll
  for (int i = 0; i < PR_TRI(N); i++, k++)
    if (LEARN) st[(size_t)k * ns] = s.P[i];
#pragma unroll
  for (int i = 0; i < N + 2; i++) st[(size_t)(k++) * ns] = s.xp[i];
  st[(size_t)(k++) * ns] = s.J;
  st[(size_t)(k++) * ns] = s.J0;
}

// slot-major state -> theta [series][n], P [series][n][n] (full), J, J0 [series]; one thread per series (a read-out, not
// a hot path: run-time indices into memory)
__global__ void k_pred_get(const double *__restrict__ state, int nseries, int n, double *__restrict__ theta,
                           double *__restrict__ P, double *__restrict__ J, double *__restrict__ J0) {
  const int S = blockIdx.x * blockDim.x + threadIdx.x;
  if (S >= nseries) return;
  const size_t ns = (size_t)nseries;
  const double *st = state + S;
  const int tri = n * (n + 1) / 2;
  if (theta)
    for (int i = 0; i < n; i++) theta[(size_t)S * n + i] = st[(size_t)i * ns];
  if (P)
    for (int i = 0; i < n; i++)
      for (int j = i; j < n; j++) {
        const double v = st[(size_t)(n + PR_IJ(n, i, j)) * ns];
        P[((size_t)S * n + i) * n + j] = v;
        P[((size_t)S * n + j) * n + i] = v;
      }
  if (J) J[S] = st[(size_t)(n + tri + n + 2) * ns];
  if (J0) J0[S] = st[(size_t)(n + tri + n + 3) * ns];
}

// ------------------------------------------------------------------------------------------------- host side
struct aomarl_predictor {
  int nenv = 0, nmodes = 0, order = 0, nseries = 0;
  long long nskip = 0;
  bool learning = true;
  PredParams par = {};
  double p0 = 0;
  PrCounts cnt;
  double *state = nullptr;                             // device [PR_SLOTS(order)][nseries]
  float *p = nullptr, *x = nullptr, *c = nullptr;      // device [nenv][nmodes]: v2m . voltage, the row consumed last, its c
  const void *owner = nullptr;                         // the context it is attached to
};

static size_t pr_slots(int n) { return (size_t)n + (size_t)n * (n + 1) / 2 + (size_t)n + 4; }

static void pr_launch(aomarl_predictor *m, const float *x, long long stride, int nframes, float *c_out, long long c_stride,
                      int c_ld, long long f0, hipStream_t s) {
  const dim3 grid((unsigned)((m->nseries + PR_BLOCK - 1) / PR_BLOCK)), blk(PR_BLOCK);
  const bool learn = m->learning, forget = m->par.forget != 1.0;
#define PR_GO(N, L, F)                                                                                                     \
  hipLaunchKernelGGL((k_pred_step<N, L, F>), grid, blk, 0, s, x, stride, nframes, m->nseries, m->nmodes, m->state, c_out, \
                     c_stride, c_ld, x == m->x ? (float *)nullptr : m->x, m->c, m->par, f0, m->nskip)
#define PR_ORDER(N)                                                              \
  case N:                                                                        \
    if (learn) { if (forget) PR_GO(N, true, true); else PR_GO(N, true, false); } \
    else { if (forget) PR_GO(N, false, true); else PR_GO(N, false, false); }     \
    break
  switch (m->order) {
    PR_ORDER(1); PR_ORDER(2); PR_ORDER(3); PR_ORDER(4); PR_ORDER(5); PR_ORDER(6); PR_ORDER(7); PR_ORDER(8);
  }
#undef PR_ORDER
#undef PR_GO
}

int aomarl_predictor_destroy(aomarl_predictor *m) {
  if (!m) return 0;
  if (m->owner) return fail("predictor_destroy: attached to a context (aomarl_predictor_attach with NULL first)");
  (void)hipDeviceSynchronize();
  void *bufs[4] = {m->state, m->p, m->x, m->c};
  for (void *b : bufs) if (b) (void)hipFree(b);
  delete m;
  return 0;
}

// theta and P of every series in the slot-major layout, from [series][n] / [series][n][n] host arrays (null: the start)
static void pr_pack(const aomarl_predictor *m, const double *theta, const double *P, std::vector<double> &out) {
  const int n = m->order;
  const size_t ns = (size_t)m->nseries, tri = (size_t)n * (n + 1) / 2;
  out.assign((n + tri) * ns, 0.0);
  for (size_t S = 0; S < ns; S++) {
    for (int i = 0; i < n; i++) out[(size_t)i * ns + S] = theta ? theta[S * n + i] : (i == 0 ? 1.0 : 0.0);
    for (int i = 0; i < n; i++)
      for (int j = i; j < n; j++)
        out[(size_t)(n + PR_IJ(n, i, j)) * ns + S] = P ? P[(S * n + i) * n + j] : (i == j ? m->p0 : 0.0);
  }
}

int aomarl_predictor_create(const aomarl_predictor_desc *d, aomarl_predictor **out) {
  if (!out) return fail("predictor_create: null argument");
  std::string err;
  if (pr_validate(d, err)) return fail("%s", err.c_str());
  aomarl_predictor *m = new aomarl_predictor();
  m->nenv = d->nenv; m->nmodes = d->nmodes; m->order = d->order; m->nseries = d->nenv * d->nmodes;
  m->nskip = d->nskip; m->p0 = d->p0;
  const double delay = (double)d->delay;
  if (delay <= 1.0) { m->par.wa = 1.0 - delay; m->par.wb = delay; m->par.wc = 0.0; }      // (mo_delay_weights' rule)
  else { m->par.wa = 0.0; m->par.wb = 2.0 - delay; m->par.wc = delay - 1.0; }
  m->par.forget = d->forget; m->par.iforget = 1.0 / d->forget; m->par.cap = (double)d->order * d->p0;
  const size_t ns = (size_t)m->nseries, sd = pr_slots(m->order) * ns;
  std::vector<double> h;
  pr_pack(m, nullptr, nullptr, h);
  bool ok = hipMalloc((void **)&m->state, sd * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&m->p, ns * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&m->x, ns * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&m->c, ns * sizeof(float)) == hipSuccess;
  ok = ok && hipMemset(m->state, 0, sd * sizeof(double)) == hipSuccess &&
       hipMemcpy(m->state, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(m->p, 0, ns * sizeof(float)) == hipSuccess && hipMemset(m->x, 0, ns * sizeof(float)) == hipSuccess &&
       hipMemset(m->c, 0, ns * sizeof(float)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    aomarl_predictor_destroy(m);
    return fail("predictor_create: device allocation failed (%d environments, %d modes, order %d)", d->nenv, d->nmodes, d->order);
  }
  *out = m;
  return 0;
}

int aomarl_predictor_restart(aomarl_predictor *m, void *stream) {
  if (!m) return fail("predictor_restart: null object");
  const int n = m->order;
  const size_t ns = (size_t)m->nseries, first = (size_t)n + (size_t)n * (n + 1) / 2;
  HIPCHK(hipMemsetAsync(m->state + first * ns, 0, (size_t)(n + 2) * ns * sizeof(double), (hipStream_t)stream));      // the past values
  m->cnt.since = 0;
  return 0;
}

int aomarl_predictor_set_learning(aomarl_predictor *m, int on) {
  if (!m) return fail("predictor_set_learning: null object");
  m->learning = on != 0;
  return 0;
}

int aomarl_predictor_push(aomarl_predictor *m, const float *x, int nframes, long long frame_stride, float *c_out, void *stream) {
  if (!m) return fail("predictor_push: null object");
  if (m->owner) return fail("predictor_push: attached to a context: aomarl_do_control feeds it");
  if (nframes < 0) return fail("predictor_push: nframes = %d", nframes);
  if (nframes == 0) return 0;
  if (!x) return fail("predictor_push: null x_dev");
  if (frame_stride < m->nseries)
    return fail("predictor_push: frame_stride = %lld is less than nenv * nmodes = %d", frame_stride, m->nseries);
  const long long f0 = pr_advance(m->cnt, nframes, m->order, m->learning);
  pr_launch(m, x, frame_stride, nframes, c_out, m->nseries, m->nmodes, f0, (hipStream_t)stream);
  LAUNCHCHK();
  return 0;
}

int aomarl_predictor_get(aomarl_predictor *m, double *theta_out, double *P_out, double *J_out, double *J0_out,
                         long long *counts_out, void *stream) {
  if (!m) return fail("predictor_get: null object");
  if (theta_out || P_out || J_out || J0_out) {
    hipLaunchKernelGGL(k_pred_get, dim3((unsigned)((m->nseries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m->state,
                       m->nseries, m->order, theta_out, P_out, J_out, J0_out);
    LAUNCHCHK();
  }
  if (counts_out) { counts_out[0] = m->cnt.total; counts_out[1] = m->cnt.since; counts_out[2] = m->cnt.learned; }
  return 0;
}

int aomarl_predictor_set(aomarl_predictor *m, const double *theta, const double *P) {
  if (!m) return fail("predictor_set: null object");
  std::string err;
  if (pr_validate_set(m->nseries, m->order, theta, P, err)) return fail("%s", err.c_str());
  if (!theta && !P) return 0;
  const int n = m->order;
  const size_t ns = (size_t)m->nseries;
  std::vector<double> h;
  pr_pack(m, theta, P, h);
  HIPCHK(hipDeviceSynchronize());
  if (theta) HIPCHK(hipMemcpy(m->state, h.data(), (size_t)n * ns * sizeof(double), hipMemcpyHostToDevice));
  if (P) HIPCHK(hipMemcpy(m->state + (size_t)n * ns, h.data() + (size_t)n * ns, (h.size() - (size_t)n * ns) * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

int aomarl_predictor_last(aomarl_predictor *m, float *x_out, float *c_out, void *stream) {
  if (!m) return fail("predictor_last: null object");
  const size_t bytes = (size_t)m->nseries * sizeof(float);
  if (x_out) HIPCHK(hipMemcpyAsync(x_out, m->x, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (c_out) HIPCHK(hipMemcpyAsync(c_out, m->c, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// ---- the pieces aomarl_do_control and aomarl_rl_control_modes run while attached (aomarl_host.h)
void pred_dims(const aomarl_predictor *m, int *nenv, int *nmodes) { *nenv = m->nenv; *nmodes = m->nmodes; }
const void *pred_owner(const aomarl_predictor *m) { return m->owner; }
void pred_set_owner(aomarl_predictor *m, const void *owner) { m->owner = owner; }
float *pred_p(aomarl_predictor *m) { return m->p; }
float *pred_x(aomarl_predictor *m) { return m->x; }
const float *pred_c(const aomarl_predictor *m) { return m->c; }

// the frame whose pseudo-open-loop modes stand in pred_x: c into pred_c and into `modes` (rows ldm apart)
int pred_frame(aomarl_predictor *m, float *modes, int ldm, hipStream_t s) {
  const long long f0 = pr_advance(m->cnt, 1, m->order, m->learning);
  pr_launch(m, m->x, m->nseries, 1, modes, 0, ldm, f0, s);
  LAUNCHCHK();
  return 0;
}
