// aomarl_modopti.hip -- modal gain optimisation (Gendron & Lena 1994, in the time domain): a bank of loop filters over
// recorded open-loop residual modes, one per (environment, mode, candidate gain).  gfx950 only.
//
// Upstream keeps its optimiser in the native library that is not part of the reference tree (init_modalOpti /
// modalControlOptimization, called from rtc_init.py:485-501); this is the published criterion -- the variance of the
// measured residual of each mode, minimised over a grid of gains -- on THIS simulator's loop (aomarl_modopti_host.h):
//     e[t] = x[t] - (wa c[t-1] + wb c[t-2] + wc c[t-3]),   c[t] = c[t-1] + g e[t],   J += e[t]^2 for t >= nskip
// No FFT, any number of frames, fed chunk by chunk while the loop records: only the filter state is kept.
//   state [4][ngain][nenv nmodes] double: c[t-1], c[t-2], c[t-3], J -- planes by gain, series contiguous, so that the 64
//         lanes of a wave read and write 512 contiguous bytes per plane
//   k_mo_bank  one workgroup = 64 adjacent series x 4 waves; wave w owns GPT gains of each of its lanes' series and keeps
//              their 4 GPT doubles in registers for the whole chunk.  The x rows of 32 frames x 64 series go through LDS
//              (each a contiguous 256-byte piece of the frame's slab), read from memory ONCE for the 4 GPT <= 32 gains
//              of a workgroup; a grid with more candidates takes one pass of x per 32 gains.  The time recursion is
//              serial; the parallelism is nenv nmodes ngain.  No atomics, no reduction: the same inputs, the same bits.
//   k_mo_result  J [env][mode][gain] and the argmin over the stable candidates, one thread per series
// The float64 statement is ao_marl_amd/modal_gains.py loop_rejection; FMA contraction is the only difference.
// On-line (aomarl_modopti_online_*, the second half of this file): the same bank fed one pseudo-open-loop row per frame
// through a device ring while the loop is closed, J = forget J + e^2 (k_mo_bank's FORGET instantiation; forget == 1 runs
// the off-line one), k_mo_pol (x = e + v2m . voltage into the ring row) and k_mo_apply (pooled argmin, G smoothed in
// double, the context's modal gains rewritten on the device).  What runs when is decided on the host from counters alone
// (mo_online_step, aomarl_modopti_host.h).  The float64 statement is modal_gains.OnlineLoopBank.
#include "aomarl_host.h"
#include "aomarl_modopti_host.h"
#include <vector>
#include <string.h>

#define MO_TS 64      // series per workgroup
#define MO_TF 32      // frames per LDS tile
#define MO_WAVES 4

// FORGET: the on-line form's J = forget J + e^2 (aomarl_modopti_online_*, forget < 1); false: the sum as it always was
template <int GPT, bool FORGET>
__global__ __launch_bounds__(256) void k_mo_bank(const float *__restrict__ x, long long stride, int nframes, long long nseries,
                                                 int ngain, const double *__restrict__ gains, double *__restrict__ state,
                                                 double wa, double wb, double wc, long long t0, long long nskip,
                                                 double forget) {
  __shared__ float xs[MO_TF][MO_TS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long s0 = (long long)blockIdx.x * MO_TS, S = s0 + lane;
  const int j0 = (int)blockIdx.y * (MO_WAVES * GPT) + wv * GPT;
  const size_t plane = (size_t)ngain * (size_t)nseries;
  double g[GPT], c0[GPT], c1[GPT], c2[GPT], J[GPT];
#pragma unroll
  for (int k = 0; k < GPT; k++) {
    const bool on = S < nseries && j0 + k < ngain;
    const size_t o = on ? (size_t)(j0 + k) * (size_t)nseries + (size_t)S : 0;
    g[k] = on ? gains[j0 + k] : 0.0;
    c0[k] = on ? state[o] : 0.0;
    c1[k] = on ? state[plane + o] : 0.0;
    c2[k] = on ? state[2 * plane + o] : 0.0;
    J[k] = on ? state[3 * plane + o] : 0.0;
  }
  for (int f0 = 0; f0 < nframes; f0 += MO_TF) {
    const int nf = nframes - f0 < MO_TF ? nframes - f0 : MO_TF;
    __syncthreads();
    for (int i = tid; i < nf * MO_TS; i += 256) {
      const int r = i >> 6, col = i & 63;
      xs[r][col] = s0 + col < nseries ? x[(long long)(f0 + r) * stride + s0 + col] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < nf; r++) {
      const double xv = (double)xs[r][lane];
      const bool on = t0 + f0 + r >= nskip;
#pragma unroll
      for (int k = 0; k < GPT; k++) {
        const double e = xv - (wa * c0[k] + wb * c1[k] + wc * c2[k]);
        const double cn = c0[k] + g[k] * e;
        if (FORGET) J[k] = on ? forget * J[k] + e * e : J[k];
        else J[k] += on ? e * e : 0.0;  // (a select, not a factor: an unstable candidate's overflow must not reach J early)
        c2[k] = c1[k]; c1[k] = c0[k]; c0[k] = cn;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < GPT; k++) {
    if (S < nseries && j0 + k < ngain) {
      const size_t o = (size_t)(j0 + k) * (size_t)nseries + (size_t)S;
      state[o] = c0[k]; state[plane + o] = c1[k]; state[2 * plane + o] = c2[k]; state[3 * plane + o] = J[k];
    }
  }
}

// J planes [gain][series] -> J_out [series][gain]; argmin over the stable candidates, ties to the lowest gain
__global__ void k_mo_result(const double *__restrict__ Jp, long long nseries, int ngain, const double *__restrict__ gains,
                            const int32_t *__restrict__ stable, double *__restrict__ J_out, int32_t *__restrict__ arg_out) {
  const long long S = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (S >= nseries) return;
  int best = -1;
  double bj = 0.0, bg = 0.0;
  for (int j = 0; j < ngain; j++) {
    const double v = Jp[(size_t)j * (size_t)nseries + (size_t)S];
    if (J_out) J_out[(size_t)S * ngain + j] = v;
    if (!stable[j]) continue;
    const double w = isfinite(v) ? v : INFINITY, gj = gains[j];
    if (best < 0 || w < bj || (w == bj && gj < bg)) { best = j; bj = w; bg = gj; }
  }
  if (arg_out) arg_out[S] = best;
}

// on-line: x = e + p, the pseudo-open-loop modes of the frame, into its ring row.  e: the residual modes -s2m . slopes
// (rows lde apart), p = v2m . voltage ([nenv][nm]).  One thread per (environment, mode).
__global__ void k_mo_pol(const float *__restrict__ e, int lde, const float *__restrict__ p, int nm, float *__restrict__ x) {
  const int r = blockIdx.y, m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nm) return;
  x[(long long)r * nm + m] = e[(long long)r * lde + m] + p[(long long)r * nm + m];
}

// on-line: the apply.  One thread per (row, mode): J of the row's environment, or the sum over the environments in
// ascending order (rows == 1 < nenv: pooled); argmin over the stable candidates by k_mo_result's rule; G smoothed in
// double, each operation rounded once (no contraction: the float64 statement's bits); mgain = float(G / gain) into the
// context's buffer where one is attached.
__global__ void k_mo_apply(const double *__restrict__ Jp, int nenv, int nm, int ngain, int rows,
                           const double *__restrict__ gains, const int32_t *__restrict__ stable, double beta,
                           double *__restrict__ G, int32_t *__restrict__ arg, float *__restrict__ mgain, double gain) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * nm) return;
  const int row = i / nm, m = i - row * nm;
  const size_t nseries = (size_t)nenv * (size_t)nm;
  int best = -1;
  double bj = 0.0, bg = 0.0;
  for (int j = 0; j < ngain; j++) {
    if (!stable[j]) continue;
    const double *Jj = Jp + (size_t)j * nseries;
    double v;
    if (rows == nenv) v = Jj[(size_t)row * nm + m];
    else {
      v = Jj[m];
      for (int e = 1; e < nenv; e++) v = v + Jj[(size_t)e * nm + m];
    }
    const double w = isfinite(v) ? v : INFINITY, gj = gains[j];
    if (best < 0 || w < bj || (w == bj && gj < bg)) { best = j; bj = w; bg = gj; }
  }
  if (best < 0) return;            // (create refuses a grid without a stable candidate)
  const double g0 = G[i];
  const double d = gains[best] - g0;
  const double bd = beta * d;
  const double g1 = g0 + bd;
  G[i] = g1;
  arg[i] = best;
  if (mgain) mgain[i] = (float)(g1 / gain);
}

// ------------------------------------------------------------------------------------------------- host side
// one launch of the bank over `nframes` rows; forget == 1: the instantiation of the off-line bank, its bits
static void mo_bank_launch(const float *x, long long stride, int nframes, long long nseries, int ngain, const double *gains,
                           double *state, double wa, double wb, double wc, long long t0, long long nskip, double forget,
                           hipStream_t s) {
  const int per = (ngain + MO_WAVES - 1) / MO_WAVES;
  const int gpt = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : 8;
  const dim3 grid((unsigned)((nseries + MO_TS - 1) / MO_TS), (unsigned)((ngain + MO_WAVES * gpt - 1) / (MO_WAVES * gpt)));
#define MO_LAUNCH(G, F)                                                                                                  \
  hipLaunchKernelGGL((k_mo_bank<G, F>), grid, dim3(256), 0, s, x, stride, nframes, nseries, ngain, gains, state, wa, wb, \
                     wc, t0, nskip, forget)
  if (forget == 1.0) {
    switch (gpt) {
      case 1: MO_LAUNCH(1, false); break;
      case 2: MO_LAUNCH(2, false); break;
      case 4: MO_LAUNCH(4, false); break;
      default: MO_LAUNCH(8, false); break;
    }
  } else {
    switch (gpt) {
      case 1: MO_LAUNCH(1, true); break;
      case 2: MO_LAUNCH(2, true); break;
      case 4: MO_LAUNCH(4, true); break;
      default: MO_LAUNCH(8, true); break;
    }
  }
#undef MO_LAUNCH
}

struct aomarl_modopti {
  int nenv, nmodes, ngain;
  long long nskip, frames, nseries;
  double wa, wb, wc;
  double *gains, *state;       // device
  int32_t *stable;             // device
  std::vector<int32_t> h_stable;
  size_t state_doubles;
};

int aomarl_modopti_destroy(aomarl_modopti *m) {
  if (!m) return 0;
  if (m->gains) (void)hipFree(m->gains);
  if (m->state) (void)hipFree(m->state);
  if (m->stable) (void)hipFree(m->stable);
  delete m;
  return 0;
}

int aomarl_modopti_reset(aomarl_modopti *m) {
  if (!m) return fail("modopti_reset: null object");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(m->state, 0, m->state_doubles * sizeof(double)));
  HIPCHK(hipDeviceSynchronize());
  m->frames = 0;
  return 0;
}

int aomarl_modopti_create(const aomarl_modopti_desc *d, aomarl_modopti **out) {
  if (!out) return fail("modopti_create: null argument");
  std::string err;
  if (mo_validate(d, err)) return fail("%s", err.c_str());
  aomarl_modopti *m = new aomarl_modopti();
  m->nenv = d->nenv; m->nmodes = d->nmodes; m->ngain = d->ngain; m->nskip = d->nskip; m->frames = 0;
  m->nseries = (long long)d->nenv * d->nmodes;
  m->gains = nullptr; m->state = nullptr; m->stable = nullptr;
  mo_delay_weights((double)d->delay, &m->wa, &m->wb, &m->wc);
  std::vector<double> hg((size_t)d->ngain);
  m->h_stable.assign((size_t)d->ngain, 0);
  for (int j = 0; j < d->ngain; j++) {
    hg[j] = (double)d->gains[j];
    m->h_stable[j] = mo_stable(hg[j], (double)d->delay) ? 1 : 0;
  }
  m->state_doubles = 4 * (size_t)d->ngain * (size_t)m->nseries;
  bool ok = hipMalloc((void **)&m->gains, hg.size() * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&m->stable, hg.size() * sizeof(int32_t)) == hipSuccess &&
            hipMalloc((void **)&m->state, m->state_doubles * sizeof(double)) == hipSuccess;
  ok = ok && hipMemcpy(m->gains, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(m->stable, m->h_stable.data(), hg.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok || aomarl_modopti_reset(m)) {
    aomarl_modopti_destroy(m);
    return fail("modopti_create: device allocation failed (%d environments, %d modes, %d gains)", d->nenv, d->nmodes, d->ngain);
  }
  *out = m;
  return 0;
}

int aomarl_modopti_accumulate(aomarl_modopti *m, const float *x, int nframes, long long frame_stride, void *stream) {
  if (!m) return fail("modopti_accumulate: null object");
  if (nframes < 0) return fail("modopti_accumulate: nframes = %d", nframes);
  if (nframes == 0) return 0;
  if (!x) return fail("modopti_accumulate: null x_dev");
  if (frame_stride < m->nseries)
    return fail("modopti_accumulate: frame_stride = %lld is less than nenv * nmodes = %lld", frame_stride, m->nseries);
  mo_bank_launch(x, frame_stride, nframes, m->nseries, m->ngain, m->gains, m->state, m->wa, m->wb, m->wc, m->frames,
                 m->nskip, 1.0, (hipStream_t)stream);
  LAUNCHCHK();
  m->frames += nframes;
  return 0;
}

int aomarl_modopti_result(aomarl_modopti *m, double *J_out, int32_t *argmin_out, int32_t *stable_out, long long *frames_out,
                          void *stream) {
  if (!m) return fail("modopti_result: null object");
  if (J_out || argmin_out) {
    hipLaunchKernelGGL(k_mo_result, dim3((unsigned)((m->nseries + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       m->state + 3 * (size_t)m->ngain * (size_t)m->nseries, m->nseries, m->ngain, m->gains, m->stable, J_out,
                       argmin_out);
    LAUNCHCHK();
  }
  if (stable_out) memcpy(stable_out, m->h_stable.data(), m->h_stable.size() * sizeof(int32_t));
  if (frames_out) *frames_out = m->frames;
  return 0;
}

// ------------------------------------------------------------------------------------------------- on-line
struct aomarl_modopti_online {
  int nenv = 0, nmodes = 0, ngain = 0, rows = 0;
  long long nseries = 0;
  double wa = 0, wb = 0, wc = 0, forget = 1.0, beta = 1.0;
  MoSchedule sch;              // every per-frame decision (aomarl_modopti_host.h)
  int last_slot = 0;
  double *gains = nullptr, *state = nullptr, *G = nullptr;     // device
  int32_t *stable = nullptr, *arg = nullptr;                   // device
  float *ring = nullptr, *p = nullptr;                         // device: [chunk][nenv][nmodes], [nenv][nmodes]
  std::vector<int32_t> h_stable;
  const void *owner = nullptr; // the context it is attached to
};

int aomarl_modopti_online_destroy(aomarl_modopti_online *m) {
  if (!m) return 0;
  if (m->owner) return fail("modopti_online_destroy: attached to a context (aomarl_modopti_online_attach with NULL first)");
  (void)hipDeviceSynchronize();
  void *bufs[7] = {m->gains, m->state, m->G, m->stable, m->arg, m->ring, m->p};
  for (void *b : bufs) if (b) (void)hipFree(b);
  delete m;
  return 0;
}

int aomarl_modopti_online_create(const aomarl_modopti_online_desc *d, aomarl_modopti_online **out) {
  if (!out) return fail("modopti_online_create: null argument");
  std::string err;
  if (mo_online_validate(d, err)) return fail("%s", err.c_str());
  aomarl_modopti_online *m = new aomarl_modopti_online();
  m->nenv = d->nenv; m->nmodes = d->nmodes; m->ngain = d->ngain; m->rows = d->pool ? 1 : d->nenv;
  m->nseries = (long long)d->nenv * d->nmodes;
  m->forget = d->forget; m->beta = d->beta;
  m->sch.chunk = d->chunk; m->sch.period = d->period; m->sch.nskip = d->nskip;
  mo_delay_weights((double)d->delay, &m->wa, &m->wb, &m->wc);
  std::vector<double> hg((size_t)d->ngain), hG((size_t)m->rows * d->nmodes, 0.0);
  m->h_stable.assign((size_t)d->ngain, 0);
  for (int j = 0; j < d->ngain; j++) {
    hg[j] = (double)d->gains[j];
    m->h_stable[j] = mo_stable(hg[j], (double)d->delay) ? 1 : 0;
  }
  if (d->G0) hG.assign(d->G0, d->G0 + hG.size());
  std::vector<int32_t> harg(hG.size(), -1);
  const size_t sd = 4 * (size_t)d->ngain * (size_t)m->nseries, ns = (size_t)m->nseries;
  bool ok = hipMalloc((void **)&m->gains, hg.size() * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&m->stable, hg.size() * sizeof(int32_t)) == hipSuccess &&
            hipMalloc((void **)&m->state, sd * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&m->G, hG.size() * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&m->arg, hG.size() * sizeof(int32_t)) == hipSuccess &&
            hipMalloc((void **)&m->ring, (size_t)d->chunk * ns * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&m->p, ns * sizeof(float)) == hipSuccess;
  ok = ok && hipMemcpy(m->gains, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(m->stable, m->h_stable.data(), hg.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(m->G, hG.data(), hG.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(m->arg, harg.data(), harg.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(m->state, 0, sd * sizeof(double)) == hipSuccess &&
       hipMemset(m->ring, 0, (size_t)d->chunk * ns * sizeof(float)) == hipSuccess &&
       hipMemset(m->p, 0, ns * sizeof(float)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    aomarl_modopti_online_destroy(m);
    return fail("modopti_online_create: device allocation failed (%d environments, %d modes, %d gains)", d->nenv, d->nmodes, d->ngain);
  }
  *out = m;
  return 0;
}

// the bank over the rows an action names
static int mo_online_consume(aomarl_modopti_online *m, const MoAction &a, hipStream_t s) {
  if (a.flush <= 0) return 0;
  mo_bank_launch(m->ring, m->nseries, a.flush, m->nseries, m->ngain, m->gains, m->state, m->wa, m->wb, m->wc, a.t0,
                 m->sch.nskip, m->forget, s);
  LAUNCHCHK();
  return 0;
}

// ---- the pieces aomarl_do_control runs while attached (aomarl_host.h); aomarl_modopti_online_push is the same two
// steps around a copy
void mo_online_dims(const aomarl_modopti_online *m, int *nenv, int *nmodes, int *rows) { *nenv = m->nenv; *nmodes = m->nmodes; *rows = m->rows; }
const void *mo_online_owner(const aomarl_modopti_online *m) { return m->owner; }
void mo_online_set_owner(aomarl_modopti_online *m, const void *owner) { m->owner = owner; }
float *mo_online_p(aomarl_modopti_online *m) { return m->p; }
static float *mo_online_slot(aomarl_modopti_online *m) { return m->ring + (size_t)m->sch.fill * (size_t)m->nseries; }

int mo_pol(const float *e, int lde, const float *p, int nenv, int nm, float *x, hipStream_t s) {
  hipLaunchKernelGGL(k_mo_pol, dim3((nm + 255) / 256, nenv), dim3(256), 0, s, e, lde, p, nm, x);
  LAUNCHCHK();
  return 0;
}

int mo_online_pol(aomarl_modopti_online *m, const float *e, int lde, hipStream_t s) {
  return mo_pol(e, lde, m->p, m->nenv, m->nmodes, mo_online_slot(m), s);
}

// the frame just written into mo_online_slot is counted; the bank and the apply follow where the schedule says so
int mo_online_advance(aomarl_modopti_online *m, float *mgain_dev, float gain, hipStream_t s, bool *applied) {
  const MoAction a = mo_online_step(m->sch);
  if (applied) *applied = a.apply;
  m->last_slot = a.slot;
  int rc = mo_online_consume(m, a, s);
  if (rc) return rc;
  if (a.apply) {
    const int n = m->rows * m->nmodes;
    hipLaunchKernelGGL(k_mo_apply, dim3((n + 255) / 256), dim3(256), 0, s,
                       m->state + 3 * (size_t)m->ngain * (size_t)m->nseries, m->nenv, m->nmodes, m->ngain, m->rows, m->gains,
                       m->stable, m->beta, m->G, m->arg, mgain_dev, (double)gain);
    LAUNCHCHK();
  }
  return 0;
}

int aomarl_modopti_online_push(aomarl_modopti_online *m, const float *x, void *stream) {
  if (!m) return fail("modopti_online_push: null object");
  if (!x) return fail("modopti_online_push: null x_dev");
  if (m->owner) return fail("modopti_online_push: attached to a context: aomarl_do_control feeds it");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(mo_online_slot(m), x, (size_t)m->nseries * sizeof(float), hipMemcpyDeviceToDevice, s));
  return mo_online_advance(m, nullptr, 1.f, s, nullptr);
}

int aomarl_modopti_online_restart(aomarl_modopti_online *m, void *stream) {
  if (!m) return fail("modopti_online_restart: null object");
  hipStream_t s = (hipStream_t)stream;
  int rc = mo_online_consume(m, mo_online_drain(m->sch), s);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(m->state, 0, 3 * (size_t)m->ngain * (size_t)m->nseries * sizeof(double), s));     // c0, c1, c2; J stays
  mo_online_restart(m->sch);
  return 0;
}

int aomarl_modopti_online_result(aomarl_modopti_online *m, double *J_out, int32_t *argmin_out, double *G_out,
                                 int32_t *stable_out, long long *counts_out, void *stream) {
  if (!m) return fail("modopti_online_result: null object");
  hipStream_t s = (hipStream_t)stream;
  int rc = mo_online_consume(m, mo_online_drain(m->sch), s);
  if (rc) return rc;
  if (J_out) {
    hipLaunchKernelGGL(k_mo_result, dim3((unsigned)((m->nseries + 255) / 256)), dim3(256), 0, s,
                       m->state + 3 * (size_t)m->ngain * (size_t)m->nseries, m->nseries, m->ngain, m->gains, m->stable, J_out,
                       (int32_t *)nullptr);
    LAUNCHCHK();
  }
  const size_t n = (size_t)m->rows * (size_t)m->nmodes;
  if (argmin_out) HIPCHK(hipMemcpyAsync(argmin_out, m->arg, n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (G_out) HIPCHK(hipMemcpyAsync(G_out, m->G, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (stable_out) memcpy(stable_out, m->h_stable.data(), m->h_stable.size() * sizeof(int32_t));
  if (counts_out) { counts_out[0] = m->sch.total; counts_out[1] = m->sch.since; counts_out[2] = m->sch.counted; counts_out[3] = m->sch.updates; }
  return 0;
}

int aomarl_modopti_online_last(aomarl_modopti_online *m, float *x_out, void *stream) {
  if (!m || !x_out) return fail("modopti_online_last: null argument");
  HIPCHK(hipMemcpyAsync(x_out, m->ring + (size_t)m->last_slot * (size_t)m->nseries, (size_t)m->nseries * sizeof(float),
                        hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}
