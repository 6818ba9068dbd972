// aomarl_roket.hip -- ROKET error breakdown (reference: guardians/roket_generalized_rl.py:189-284, 441-480): the loop
// filters of the seven contributors and the modal moments of their covariance table, for all environments at once.
// gfx950 only.
//
// The reference keeps [n_iter][nactu] histories of every buffer and filters them on the host.  Here one object keeps,
// per environment, only what frame t reads:
//   X    [7][nenv][ld]         x_k[t-1] -> x_k[t], k = noise, trunc, alias, H_com, bp, tomo, zeta (the cov_cor order);
//                              as it lies the operand of  Y = X P^T  ([7 nenv, nactu] against P)
//   ring [delay] slots, slot t mod delay written at frame t, read at frame t + delay:
//     op [6][nenv][ld]         x_k[t] of the six filtered contributors (noise, trunc, alias, bp, tomo, zeta), the tomo
//                              row holding x_tomo[t] + tomo_buf[t]: gRD (x_tomo + tomo_buf) is the reference's
//                              gRD x_tomo[t-d] + g gamma RD tomo_buf[t-d]; as it lies the operand of  R = op gRD^T
//     u  [4][nenv][ld]         noise_buf, trunc_buf, ageom, rl_com of frame t
//   bufs [4][nenv][ld]         noise_buf, trunc_buf, tomo_buf, mod_com of the last frame (mod_com[t-1] of the next)
// A step is five products on the library's fp32 GEMM (aomarl_gemm_nt: no split-K, so a fixed summation order) with the
// kernels of this file around them:
//   k_rk_pack    B, G -> [2 nenv][ld]                       modes = . P^T
//   k_rk_split   modes -> filt(B), rest(B), rest(G)         H_com, mod_com, wf_com = . Btt^T
//                                                           R = op[t - delay] gRD^T
//   k_rk_update  the six recursions, H_com, the ring slot and bufs of frame t
//                                                           Y = X P^T
//   k_rk_moments S1[env][k][m] += y_k, S2[env][k <= l][m] += y_k y_l in double: one thread owns one (env, mode) and
//                adds its 35 sums itself, so there is no reduction, no atomic, and two runs give the same bits.
// History before frame 0 is zero (the reference indexes its zero-filled buffers at -1, -delay).
#include "aomarl_host.h"
#include <vector>
#include <string.h>

#define RK_NC 7      // contributors
#define RK_NF 6      // filtered contributors (all but H_com)
#define RK_NP 28     // pairs k <= l

// --------------------------------------------------------------------------------------------------- kernels
__global__ void k_rk_pack(const float *__restrict__ B, const float *__restrict__ G, int ld_in, float *__restrict__ out,
                          int nenv, int nactu, int ld) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)nenv * nactu;
  if (i >= per * (G ? 2 : 1)) return;
  const int which = (int)(i / per);
  const long long j = i - which * per;
  const int e = (int)(j / nactu), a = (int)(j - (long long)e * nactu);
  out[((size_t)which * nenv + e) * ld + a] = (which ? G : B)[(size_t)e * ld_in + a];
}

// modes [nin nenv][ldm] (B rows, then G rows) -> m3 [(1 + nin) nenv][ldm]: filt(B), rest(B), rest(G)
// filt keeps the modes [lo, hi) = [-nfiltered-2 : -2], rest zeroes them (roket_generalized_rl.py:258-264, 277-279)
__global__ void k_rk_split(const float *__restrict__ modes, float *__restrict__ m3, int nenv, int nmodes, int ldm, int lo,
                           int hi, int nin) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)nenv * nmodes;
  if (i >= per * nin) return;
  const int which = (int)(i / per);
  const long long j = i - which * per;
  const int e = (int)(j / nmodes), m = (int)(j - (long long)e * nmodes);
  const float v = modes[((size_t)which * nenv + e) * ldm + m];
  const bool filt = m >= lo && m < hi;
  if (which == 0) {
    m3[(size_t)e * ldm + m] = filt ? v : 0.f;
    m3[((size_t)nenv + e) * ldm + m] = filt ? 0.f : v;
  } else {
    m3[((size_t)2 * nenv + e) * ldm + m] = filt ? 0.f : v;
  }
}

struct RkUpd {
  const float *derr, *E, *F, *ageom, *rl;   // [nenv][ld_in]; rl may be NULL
  int ld_in;
  const float *v3;     // [3 nenv][ld]: H_com, mod_com, wf_com (wf_com absent when !has_g)
  const float *R;      // [6 nenv][ld]
  float *X;            // [7 nenv][ld]
  float *op, *u;       // ring slot of this frame: [6 nenv][ld], [4 nenv][ld]
  float *bufs;         // [4 nenv][ld]
  int nenv, nactu, ld, has_g;
  float g, gamma;
};

// one thread per (env, actuator).  The slot it overwrites is the one whose op fed R and whose u it reads first.
__global__ void k_rk_update(RkUpd p) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)p.nenv * p.nactu) return;
  const int e = (int)(i / p.nactu), a = (int)(i - (long long)e * p.nactu);
  const size_t in = (size_t)e * p.ld_in + a, o = (size_t)e * p.ld + a, row = (size_t)p.nenv * p.ld;
  const float derr = p.derr[in], E = p.E[in], F = p.F[in], ag = p.ageom[in], rl = p.rl ? p.rl[in] : 0.f;
  const float hcom = p.v3[o], mod = p.v3[row + o], wf = p.has_g ? p.v3[2 * row + o] : mod;
  const float u_noise = p.u[o], u_trunc = p.u[row + o], u_alias = p.u[2 * row + o], u_rl = p.u[3 * row + o];
  const float mod_prev = p.bufs[3 * row + o];
  const float noise_buf = derr - E, trunc_buf = E - p.gamma * F, tomo_buf = p.has_g ? mod - wf : 0.f;
  // x[t] = x[t-1] - gRD x[t-delay] + u[t-delay], evaluated left to right as the reference's expressions are
  const float x_noise = p.X[o] - p.R[o] + p.g * u_noise;                              // :217-218
  const float x_trunc = p.X[row + o] - p.R[row + o] + p.g * u_trunc;                  // :230-231
  const float x_alias = p.X[2 * row + o] - p.R[2 * row + o] + p.gamma * p.g * u_alias;// :245-247
  const float x_bp = p.X[4 * row + o] - p.R[3 * row + o] - (mod - mod_prev);          // :267-269: C[t], undelayed
  const float x_tomo = p.X[5 * row + o] - p.R[4 * row + o];                           // :282-284: R holds both terms
  const float x_zeta = p.X[6 * row + o] - p.R[5 * row + o] + u_rl;                    // :190-192
  p.X[o] = x_noise;
  p.X[row + o] = x_trunc;
  p.X[2 * row + o] = x_alias;
  p.X[3 * row + o] = hcom;
  p.X[4 * row + o] = x_bp;
  p.X[5 * row + o] = x_tomo;
  p.X[6 * row + o] = x_zeta;
  p.op[o] = x_noise;
  p.op[row + o] = x_trunc;
  p.op[2 * row + o] = x_alias;
  p.op[3 * row + o] = x_bp;
  p.op[4 * row + o] = x_tomo + tomo_buf;
  p.op[5 * row + o] = x_zeta;
  p.u[o] = noise_buf;
  p.u[row + o] = trunc_buf;
  p.u[2 * row + o] = ag;
  p.u[3 * row + o] = rl;
  p.bufs[o] = noise_buf;
  p.bufs[row + o] = trunc_buf;
  p.bufs[2 * row + o] = tomo_buf;
  p.bufs[3 * row + o] = mod;
}

// Y [7 nenv][ldm] -> S1 [nenv][7][nmodes], S2 [nenv][28][nmodes] (pairs k <= l, k major), double
__global__ void k_rk_moments(const float *__restrict__ Y, double *__restrict__ S1, double *__restrict__ S2, int nenv,
                             int nmodes, int ldm) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)nenv * nmodes) return;
  const int e = (int)(i / nmodes), m = (int)(i - (long long)e * nmodes);
  double y[RK_NC];
#pragma unroll
  for (int k = 0; k < RK_NC; k++) y[k] = (double)Y[((size_t)k * nenv + e) * ldm + m];
  double *s1 = S1 + (size_t)e * RK_NC * nmodes + m;
  double *s2 = S2 + (size_t)e * RK_NP * nmodes + m;
  int pr = 0;
#pragma unroll
  for (int k = 0; k < RK_NC; k++) {
    s1[(size_t)k * nmodes] += y[k];
#pragma unroll
    for (int l = k; l < RK_NC; l++, pr++) s2[(size_t)pr * nmodes] += y[k] * y[l];
  }
}

// [rows][nenv][ld] -> [rows][nenv][nactu]
__global__ void k_rk_unpad(const float *__restrict__ src, float *__restrict__ dst, long long nrow, int n, int ld) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrow * n) return;
  const long long r = i / n;
  dst[i] = src[(size_t)r * ld + (i - r * n)];
}

// ------------------------------------------------------------------------------------------------- host side
struct aomarl_roket {
  int nenv, nactu, ld_in, nmodes, nfiltered, delay, ld, ldm;
  float g, gamma;
  long long t, frames;
  float *gRD, *P, *Btt;                       // device, rows padded to ld / ld / ldm
  float *X, *ring, *bufs, *bg, *modes, *m3, *v3, *R, *Y;
  double *S1, *S2;
  size_t slot_floats, ring_floats;
};

static inline unsigned rk_blocks(long long total) { return (unsigned)((total + 255) / 256); }

int aomarl_roket_destroy(aomarl_roket *r) {
  if (!r) return 0;
  void *p[] = {r->gRD, r->P, r->Btt, r->X, r->ring, r->bufs, r->bg, r->modes, r->m3, r->v3, r->R, r->Y, r->S1, r->S2};
  for (void *q : p) if (q) (void)hipFree(q);
  delete r;
  return 0;
}

int aomarl_roket_reset(aomarl_roket *r) {
  if (!r) return fail("roket_reset: null object");
  const size_t rows = (size_t)r->nenv * r->ld;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(r->X, 0, RK_NC * rows * sizeof(float)));
  HIPCHK(hipMemset(r->ring, 0, r->ring_floats * sizeof(float)));
  HIPCHK(hipMemset(r->bufs, 0, 4 * rows * sizeof(float)));
  HIPCHK(hipMemset(r->S1, 0, (size_t)r->nenv * RK_NC * r->nmodes * sizeof(double)));
  HIPCHK(hipMemset(r->S2, 0, (size_t)r->nenv * RK_NP * r->nmodes * sizeof(double)));
  HIPCHK(hipDeviceSynchronize());
  r->t = 0;
  r->frames = 0;
  return 0;
}

int aomarl_roket_create(const aomarl_roket_desc *d, aomarl_roket **out) {
  if (!d || !out) return fail("roket_create: null argument");
  if (!d->RD || !d->P || !d->Btt) return fail("roket_create: null matrix");
  if (d->nenv < 1 || d->nactu < 1 || d->nmodes < 1 || d->ld_actu < d->nactu)
    return fail("roket_create: nenv %d nactu %d ld_actu %d nmodes %d", d->nenv, d->nactu, d->ld_actu, d->nmodes);
  if (d->nfiltered < 0 || d->nfiltered + 2 > d->nmodes)
    return fail("roket_create: nfiltered %d of %d modes (the last two are tip and tilt)", d->nfiltered, d->nmodes);
  if (d->delay < 1 || d->delay > 64) return fail("roket_create: delay %d (int(controller delay) + 1, 1..64)", d->delay);
  aomarl_roket *r = new aomarl_roket();
  memset(r, 0, sizeof(*r));
  r->nenv = d->nenv; r->nactu = d->nactu; r->ld_in = d->ld_actu; r->nmodes = d->nmodes;
  r->nfiltered = d->nfiltered; r->delay = d->delay; r->g = d->g; r->gamma = d->gamma;
  r->ld = (d->nactu + 3) & ~3;
  r->ldm = (d->nmodes + 3) & ~3;
  const int na = r->nactu, nm = r->nmodes, ld = r->ld, ldm = r->ldm;
  const size_t rows = (size_t)r->nenv * ld, mrows = (size_t)r->nenv * ldm;
  r->slot_floats = (RK_NF + 4) * rows;
  r->ring_floats = r->slot_floats * r->delay;
  std::vector<float> hRD((size_t)na * ld, 0.f), hP((size_t)nm * ld, 0.f), hB((size_t)na * ldm, 0.f);
  const float gg = d->g * d->gamma;   // self.gRD = gain * gamma * RD (:161)
  for (int i = 0; i < na; i++)
    for (int j = 0; j < na; j++) hRD[(size_t)i * ld + j] = gg * d->RD[(size_t)i * na + j];
  for (int i = 0; i < nm; i++)
    for (int j = 0; j < na; j++) hP[(size_t)i * ld + j] = d->P[(size_t)i * na + j];
  for (int i = 0; i < na; i++)
    for (int j = 0; j < nm; j++) hB[(size_t)i * ldm + j] = d->Btt[(size_t)i * nm + j];
  bool ok = hipMalloc((void **)&r->gRD, hRD.size() * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->P, hP.size() * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->Btt, hB.size() * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->X, RK_NC * rows * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->ring, r->ring_floats * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->bufs, 4 * rows * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->bg, 2 * rows * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->modes, 2 * mrows * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->m3, 3 * mrows * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->v3, 3 * rows * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->R, RK_NF * rows * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->Y, RK_NC * mrows * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->S1, (size_t)r->nenv * RK_NC * nm * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&r->S2, (size_t)r->nenv * RK_NP * nm * sizeof(double)) == hipSuccess;
  // the pad columns of every operand are never read (K = nactu or nmodes), but nothing is left uninitialised
  ok = ok && hipMemcpy(r->gRD, hRD.data(), hRD.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->P, hP.data(), hP.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->Btt, hB.data(), hB.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(r->bg, 0, 2 * rows * sizeof(float)) == hipSuccess &&
       hipMemset(r->modes, 0, 2 * mrows * sizeof(float)) == hipSuccess &&
       hipMemset(r->m3, 0, 3 * mrows * sizeof(float)) == hipSuccess &&
       hipMemset(r->v3, 0, 3 * rows * sizeof(float)) == hipSuccess &&
       hipMemset(r->R, 0, RK_NF * rows * sizeof(float)) == hipSuccess &&
       hipMemset(r->Y, 0, RK_NC * mrows * sizeof(float)) == hipSuccess;
  if (!ok || aomarl_roket_reset(r)) {
    aomarl_roket_destroy(r);
    return fail("roket_create: device allocation failed (%d environments, %d actuators, %d modes, delay %d)", d->nenv,
                d->nactu, d->nmodes, d->delay);
  }
  *out = r;
  return 0;
}

int aomarl_roket_step(aomarl_roket *r, const float *derr, const float *E, const float *F, const float *ageom,
                      const float *B, const float *G, const float *rl_com, int accumulate, void *stream) {
  if (!r) return fail("roket_step: null object");
  if (!derr || !E || !F || !ageom || !B) return fail("roket_step: null input (only G and rl_com may be NULL)");
  hipStream_t s = (hipStream_t)stream;
  const int nenv = r->nenv, na = r->nactu, nm = r->nmodes, ld = r->ld, ldm = r->ldm, nin = G ? 2 : 1;
  const size_t rows = (size_t)nenv * ld;
  const int lo = nm - r->nfiltered - 2, hi = nm - 2;
  k_rk_pack<<<rk_blocks((long long)nin * nenv * na), 256, 0, s>>>(B, G, r->ld_in, r->bg, nenv, na, ld);
  LAUNCHCHK();
  if (aomarl_gemm_nt(nin * nenv, nm, na, 1.f, r->bg, ld, r->P, ld, 0.f, r->modes, ldm, s)) return 1;
  k_rk_split<<<rk_blocks((long long)nin * nenv * nm), 256, 0, s>>>(r->modes, r->m3, nenv, nm, ldm, lo, hi, nin);
  LAUNCHCHK();
  if (aomarl_gemm_nt((1 + nin) * nenv, na, nm, 1.f, r->m3, ldm, r->Btt, ldm, 0.f, r->v3, ld, s)) return 1;
  float *slot = r->ring + (size_t)(r->t % r->delay) * r->slot_floats;   // frame t - delay's, frame t's after the update
  if (aomarl_gemm_nt(RK_NF * nenv, na, na, 1.f, slot, ld, r->gRD, ld, 0.f, r->R, ld, s)) return 1;
  RkUpd p;
  p.derr = derr; p.E = E; p.F = F; p.ageom = ageom; p.rl = rl_com; p.ld_in = r->ld_in;
  p.v3 = r->v3; p.R = r->R; p.X = r->X; p.op = slot; p.u = slot + RK_NF * rows; p.bufs = r->bufs;
  p.nenv = nenv; p.nactu = na; p.ld = ld; p.has_g = G ? 1 : 0; p.g = r->g; p.gamma = r->gamma;
  k_rk_update<<<rk_blocks((long long)nenv * na), 256, 0, s>>>(p);
  LAUNCHCHK();
  r->t++;
  if (accumulate) {
    if (aomarl_gemm_nt(RK_NC * nenv, nm, na, 1.f, r->X, ld, r->P, ld, 0.f, r->Y, ldm, s)) return 1;
    k_rk_moments<<<rk_blocks((long long)nenv * nm), 256, 0, s>>>(r->Y, r->S1, r->S2, nenv, nm, ldm);
    LAUNCHCHK();
    r->frames++;
  }
  return 0;
}

int aomarl_roket_moments(aomarl_roket *r, double *S1_out, double *S2_out, long long *frames_out, void *stream) {
  if (!r) return fail("roket_moments: null object");
  hipStream_t s = (hipStream_t)stream;
  if (S1_out) HIPCHK(hipMemcpyAsync(S1_out, r->S1, (size_t)r->nenv * RK_NC * r->nmodes * sizeof(double),
                                    hipMemcpyDeviceToDevice, s));
  if (S2_out) HIPCHK(hipMemcpyAsync(S2_out, r->S2, (size_t)r->nenv * RK_NP * r->nmodes * sizeof(double),
                                    hipMemcpyDeviceToDevice, s));
  if (frames_out) *frames_out = r->frames;
  return 0;
}

int aomarl_roket_history(aomarl_roket *r, float *x_out, float *bufs_out, void *stream) {
  if (!r) return fail("roket_history: null object");
  hipStream_t s = (hipStream_t)stream;
  const long long nrow = (long long)r->nenv;
  if (x_out) {
    k_rk_unpad<<<rk_blocks(RK_NC * nrow * r->nactu), 256, 0, s>>>(r->X, x_out, RK_NC * nrow, r->nactu, r->ld);
    LAUNCHCHK();
  }
  if (bufs_out) {
    k_rk_unpad<<<rk_blocks(4 * nrow * r->nactu), 256, 0, s>>>(r->bufs, bufs_out, 4 * nrow, r->nactu, r->ld);
    LAUNCHCHK();
  }
  return 0;
}
