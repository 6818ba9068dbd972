// aomarl_tomo.hip -- laser tomography (include/aomarl.h: aomarl_tomo_*).  gfx950 only.
// The model is ao_marl_amd/tomography.py (tomo_trace_model, slope_covariance; float64 NumPy).  A translation unit of its
// own, like aomarl_lgs.hip: the trace reads the context's static description and the state through aomarl_env_host.h.  The
// host half is aomarl_tomo_host.h.
#include "aomarl_env_host.h"
#include "aomarl_trace_dev.h"
#include "aomarl_tomo_host.h"

// =============================================================================================
// k_tomo_trace: k_lgs_trace for every star of an environment in one launch.  k_raytrace's shape: a workgroup owns 256
// consecutive pixels, a thread one pixel and, here, that pixel of all K planes.  The star loop sits inside the layer
// loop: a layer's rows are fetched once per workgroup (the stars' footprints overlap, the second star finds them in the
// cache) and the layer's constants are read once.  The stars' sums live in K named registers (the loop over k is
// unrolled to AOMARL_TOMO_MAX_STARS and predicated: no run-time index into a register array).  off and dm1 ride in the
// kernel's arguments (uniform: scalar registers).  The mirrors sit in the pupil, their value at a pixel is the same for
// every star: each is evaluated once per pixel (trace_dm_values) and added to every star's sum in controller order,
// after the layers -- per plane the operations and their order are k_lgs_trace's, so the bits are.
// =============================================================================================
struct TomoArgs {
  float ox[AOMARL_MAX_LAYERS][AOMARL_TOMO_MAX_STARS], oy[AOMARL_MAX_LAYERS][AOMARL_TOMO_MAX_STARS];
  float dm1[AOMARL_MAX_LAYERS][AOMARL_TOMO_MAX_STARS];
};

__global__ __launch_bounds__(256) void k_tomo_trace(DevSys sys, DevState st, TomoArgs a, int K, float *__restrict__ planes,
                                                    int env_begin, int flags) {
  const int nn = sys.n;
  const int e = env_begin + blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nn * nn) return;
  const int y = p / nn, x = p - y * nn;
  float *out = planes + (long long)e * K * nn * nn + p;          // plane k of the environment: out[k nn nn]
  float v[AOMARL_TOMO_MAX_STARS];
#pragma unroll
  for (int k = 0; k < AOMARL_TOMO_MAX_STARS; k++)
    v[k] = (k < K && !(flags & AOMARL_TRACE_RESET)) ? out[(long long)k * nn * nn] : 0.f;
  if (flags & AOMARL_TRACE_ATMOS) {
    const float c = 0.5f * (float)(nn - 1);
    const float dx = (float)x - c, dy = (float)y - c;      // exact: half-integers below 2^23
    for (int l = 0; l < sys.nlayers; l++) {
      const DevLayer &L = sys.layers[l];
      const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
      const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
#pragma unroll
      for (int k = 0; k < AOMARL_TOMO_MAX_STARS; k++)
        if (k < K)
          v[k] += bilinear_ring(base, L.dim, ox, oy, __fmaf_rn(a.dm1[l][k], dx, (float)x + a.ox[l][k]),
                                __fmaf_rn(a.dm1[l][k], dy, (float)y + a.oy[l][k]));
    }
  }
  if (flags & AOMARL_TRACE_DMS) {
    float dmv[AOMARL_MAX_DMS];
    const unsigned has = trace_dm_values(sys, st, e, x, y, dmv);
#pragma unroll
    for (int m = 0; m < AOMARL_MAX_DMS; m++)
      if (has & (1u << m)) {
#pragma unroll
        for (int k = 0; k < AOMARL_TOMO_MAX_STARS; k++) v[k] += dmv[m];
      }
  }
  const float mk = (flags & AOMARL_TRACE_MASK) ? sys.mpupil[p] : 1.f;
#pragma unroll
  for (int k = 0; k < AOMARL_TOMO_MAX_STARS; k++)
    if (k < K) out[(long long)k * nn * nn] = (flags & AOMARL_TRACE_MASK) ? v[k] * mk : v[k];
}

// =============================================================================================
// k_tomo_cov: one element of the covariance per thread, in double (tomo_cov_entry, aomarl_tomo_host.h: layers outer,
// then the four taps; rodconan is aomarl_groot_fn.h's).  A workgroup owns a 16 x 16 tile of the [2 n_a K_a][2 n_b K_b]
// matrix; the (star, layer) tables (at most 8 x 8 x 24 bytes per side) are staged in LDS.  Row r = (2 a + e) n_a + i.
// The structure function is long double-precision arithmetic (three pow, a ten-term series): the kernel is bound by
// the vector unit, not by memory; no symmetry or lag table is used.  No atomics, nothing depends on the launch.
// =============================================================================================
__global__ __launch_bounds__(TOMO_THREADS) void k_tomo_cov(const double *__restrict__ rpx, const double *__restrict__ rpy,
                                                           int n_row, int k_row, const double *__restrict__ cpx,
                                                           const double *__restrict__ cpy, int n_col, int k_col,
                                                           const TomoStarLayer *__restrict__ rtab,
                                                           const TomoStarLayer *__restrict__ ctab,
                                                           const TomoLayer *__restrict__ lay, int nlayers, double d,
                                                           double *__restrict__ out) {
  __shared__ TomoStarLayer srow[AOMARL_TOMO_MAX_STARS * TOMO_MAX_LAYERS], scol[AOMARL_TOMO_MAX_STARS * TOMO_MAX_LAYERS];
  __shared__ TomoLayer slay[TOMO_MAX_LAYERS];
  const int tid = threadIdx.y * TOMO_TILE + threadIdx.x;
  if (tid < k_row * nlayers) srow[tid] = rtab[tid];
  if (tid < k_col * nlayers) scol[tid] = ctab[tid];
  if (tid < nlayers) slay[tid] = lay[tid];
  __syncthreads();
  const long long R = 2LL * n_row * k_row, Cn = 2LL * n_col * k_col;
  const long long r = (long long)blockIdx.y * TOMO_TILE + threadIdx.y, c = (long long)blockIdx.x * TOMO_TILE + threadIdx.x;
  if (r >= R || c >= Cn) return;
  const int ga = (int)(r / n_row), i = (int)(r - (long long)ga * n_row), gb = (int)(c / n_col), j = (int)(c - (long long)gb * n_col);
  out[r * Cn + c] = tomo_cov_entry(rpx[i], rpy[i], srow + (ga >> 1) * nlayers, ga & 1, cpx[j], cpy[j],
                                   scol + (gb >> 1) * nlayers, gb & 1, slay, nlayers, d);
}

// ------------------------------------------------------------------------------------------------- host side
int aomarl_tomo_trace(aomarl_ctx *c, aomarl_state *st, const aomarl_tomo_desc *d, float *planes, int b, int n, int flags,
                      void *stream) {
  if (!c || !st) return fail("tomo_trace: null argument");
  int rc = env_refuse_busy("tomo_trace", c);
  if (rc) return rc;
  const EnvView v = env_view(c);
  std::string err;
  const int known = AOMARL_TRACE_ATMOS | AOMARL_TRACE_DMS | AOMARL_TRACE_RESET | AOMARL_TRACE_MASK;
  int dims[AOMARL_MAX_LAYERS];
  for (int l = 0; l < AOMARL_MAX_LAYERS; l++) dims[l] = l < v.nlayers ? v.sys.layers[l].dim : 0;
  if (tomo_validate_trace(d, planes, v.nlayers, dims, v.sys.n, st->nenv, b, n, flags, known, err))
    return fail("%s", err.c_str());
  rc = env_trace_ready(c, st, b, n, flags, stream);
  if (rc) return rc;
  TomoArgs a;
  memset(&a, 0, sizeof(a));
  for (int l = 0; l < d->nlayers; l++)
    for (int k = 0; k < d->nstars; k++) {
      const float *o = d->off + 2 * (k * d->nlayers + l);
      a.ox[l][k] = v.frac_x ? o[0] + v.frac_x[l] : o[0];
      a.oy[l][k] = v.frac_y ? o[1] + v.frac_y[l] : o[1];
      a.dm1[l][k] = d->dm1[k * d->nlayers + l];
    }
  const int np = v.sys.n * v.sys.n;
  hipLaunchKernelGGL(k_tomo_trace, dim3((np + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, v.sys, dev_state(st), a,
                     d->nstars, planes, b, flags);
  LAUNCHCHK();
  return 0;
}

int aomarl_tomo_cov(const aomarl_tomo_cov_desc *d, double *out, void *stream) {
  std::string err;
  if (tomo_validate_cov(d, out, err)) return fail("%s", err.c_str());
  std::vector<TomoStarLayer> rows, cols;
  std::vector<TomoLayer> lay;
  tomo_cov_tables(d, rows, cols, lay);
  hipStream_t s = (hipStream_t)stream;
  const size_t bp_r = (size_t)d->n_row * sizeof(double), bp_c = (size_t)d->n_col * sizeof(double);
  const size_t bt_r = rows.size() * sizeof(TomoStarLayer), bt_c = cols.size() * sizeof(TomoStarLayer);
  const size_t bl = lay.size() * sizeof(TomoLayer);
  // one allocation: [row px | row py | col px | col py | row table | col table | layers], all multiples of 8 bytes
  char *buf = nullptr;
  HIPCHK(hipMalloc((void **)&buf, 2 * bp_r + 2 * bp_c + bt_r + bt_c + bl));
  char *q = buf;
  const void *src[7] = {d->row_px, d->row_py, d->col_px, d->col_py, rows.data(), cols.data(), lay.data()};
  const size_t len[7] = {bp_r, bp_r, bp_c, bp_c, bt_r, bt_c, bl};
  char *at[7];
  bool ok = true;
  for (int i = 0; i < 7; i++) {
    at[i] = q;
    ok = ok && hipMemcpyAsync(q, src[i], len[i], hipMemcpyHostToDevice, s) == hipSuccess;
    q += len[i];
  }
  ok = ok && hipStreamSynchronize(s) == hipSuccess;       // (the host arrays are pageable: the copies have read them)
  if (ok) {
    const long long R = 2LL * d->n_row * d->k_row, Cn = 2LL * d->n_col * d->k_col;
    k_tomo_cov<<<dim3((unsigned)((Cn + TOMO_TILE - 1) / TOMO_TILE), (unsigned)((R + TOMO_TILE - 1) / TOMO_TILE)),
                 dim3(TOMO_TILE, TOMO_TILE), 0, s>>>((const double *)at[0], (const double *)at[1], d->n_row, d->k_row,
                                                      (const double *)at[2], (const double *)at[3], d->n_col, d->k_col,
                                                      (const TomoStarLayer *)at[4], (const TomoStarLayer *)at[5],
                                                      (const TomoLayer *)at[6], d->nlayers, d->d, out);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  }
  (void)hipFree(buf);
  if (!ok) return fail("tomo_cov: copy or launch failed (%d x %d points)", d->n_row, d->n_col);
  return 0;
}
