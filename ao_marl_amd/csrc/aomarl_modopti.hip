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
#include "aomarl_host.h"
#include "aomarl_modopti_host.h"
#include <vector>
#include <string.h>

#define MO_TS 64      // series per workgroup
#define MO_TF 32      // frames per LDS tile
#define MO_WAVES 4

template <int GPT>
__global__ __launch_bounds__(256) void k_mo_bank(const float *__restrict__ x, long long stride, int nframes, long long nseries,
                                                 int ngain, const double *__restrict__ gains, double *__restrict__ state,
                                                 double wa, double wb, double wc, long long t0, long long nskip) {
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
        J[k] += on ? e * e : 0.0;       // (a select, not a factor: an unstable candidate's overflow must not reach J early)
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

// ------------------------------------------------------------------------------------------------- host side
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
  hipStream_t s = (hipStream_t)stream;
  const int per = (m->ngain + MO_WAVES - 1) / MO_WAVES;
  const int gpt = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : 8;
  const dim3 grid((unsigned)((m->nseries + MO_TS - 1) / MO_TS), (unsigned)((m->ngain + MO_WAVES * gpt - 1) / (MO_WAVES * gpt)));
#define MO_LAUNCH(G)                                                                                                     \
  hipLaunchKernelGGL(k_mo_bank<G>, grid, dim3(256), 0, s, x, frame_stride, nframes, m->nseries, m->ngain, m->gains,      \
                     m->state, m->wa, m->wb, m->wc, m->frames, m->nskip)
  switch (gpt) {
    case 1: MO_LAUNCH(1); break;
    case 2: MO_LAUNCH(2); break;
    case 4: MO_LAUNCH(4); break;
    default: MO_LAUNCH(8); break;
  }
#undef MO_LAUNCH
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
