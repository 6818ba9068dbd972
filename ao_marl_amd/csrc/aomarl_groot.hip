// aomarl_groot.hip -- the GROOT covariance model (reference: guardians/groot.py compute_Cerr_cpu :110-212,
// compute_Calias :533-609, compute_dCmm :792-903; structure functions guardians/starlord.py:10-140).  gfx950 only.
//
//   k_groot_form     out[b][i][j] = sum_t w[b][t] F_kind(t)(|p_j - p_i + o[b][t]|; x0, L0[b][t]).  One thread per (i, j),
//                    16 x 16 pairs per workgroup, grid (column tiles, row tiles, batch).  The model is a second difference
//                    of structure functions that are 10^2 - 10^3 times larger than the result at 8 m separations (L0 =
//                    1e5 m in production), so F and the tap sum are double and only out is rounded to float.  The taps of
//                    the workgroup's batch entry are staged in LDS; the Ij0 table (160 KB) is read through L2: a wave's
//                    64 separations fall into a handful of neighbouring table intervals.
//   k_groot_reduce   the fixed-order sum of a product's k-split slabs
// The sandwich G C G^T runs on k_gemm_p (aomarl_gemm_p.h, through the environment unit's gemm_p_launch_cfg), twice:
// T = G C^T, out = G T^T.
#include "aomarl_host.h"
#include "aomarl_gemm_p_host.h"   // GemmPCfg, gemm_p_pick
#include "aomarl_groot_host.h"
#include <string.h>

#define GR_TILE 16
#define GR_MAX_TAPS (6 * GR_MAX_LAYERS)      // per batch entry: 18 KB of LDS at the most

__global__ __launch_bounds__(GR_TILE * GR_TILE) void k_groot_form(const double *__restrict__ px, const double *__restrict__ py,
                                                                   int n, const GrTap *__restrict__ taps, int ntaps,
                                                                   const double *__restrict__ tabx,
                                                                   const double *__restrict__ taby, float *__restrict__ out,
                                                                   int ldo, long long stride_o) {
  __shared__ GrTap st[GR_MAX_TAPS];
  const int tid = threadIdx.y * GR_TILE + threadIdx.x, b = blockIdx.z;
  for (int t = tid; t < ntaps; t += GR_TILE * GR_TILE) st[t] = taps[(size_t)b * ntaps + t];
  __syncthreads();
  const int j = blockIdx.x * GR_TILE + threadIdx.x, i = blockIdx.y * GR_TILE + threadIdx.y;
  if (i >= n || j >= n) return;
  const double dx = px[j] - px[i], dy = py[j] - py[i];
  double acc = 0.0;
  for (int t = 0; t < ntaps; t++) {
    const double x = dx + st[t].ox, y = dy + st[t].oy;
    acc += st[t].w * gr_eval(st[t].kind, sqrt(x * x + y * y), st[t].x0, st[t].L0, tabx, taby);
  }
  out[(size_t)b * stride_o + (size_t)i * ldo + j] = (float)acc;
}

// C[m][n] = (add ? C : 0) + P[0] + P[1] + ... in that order
__global__ void k_groot_reduce(int M, int N, int nz, const float *__restrict__ P, float *__restrict__ C, int ldc, int add) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)M * N) return;
  const int row = (int)(i / N), col = (int)(i - (long long)row * N);
  float *c = C + (size_t)row * ldc + col;
  float s = add ? *c : 0.f;
  for (int z = 0; z < nz; z++) s += P[(size_t)z * M * N + i];
  *c = s;
}

// ------------------------------------------------------------------------------------------------- host side
#define GR_MAX_SPLIT 8
struct aomarl_groot {
  int n_max, batch_max, m_max, k_max, ldt;
  size_t ws_floats;
  double *tabx, *taby;
  GrTap *taps, *taps_host;     // device buffer and its pinned staging copy
  hipEvent_t staged;           // behind the last kernel that read `taps`: both buffers are free again
  float *T, *ws;
};

int aomarl_groot_destroy(aomarl_groot *g) {
  if (!g) return 0;
  void *q[] = {g->tabx, g->taby, g->taps, g->T, g->ws};
  for (void *v : q) if (v) (void)hipFree(v);
  if (g->taps_host) (void)hipHostFree(g->taps_host);
  if (g->staged) (void)hipEventDestroy(g->staged);
  delete g;
  return 0;
}

int aomarl_groot_create(const aomarl_groot_desc *d, aomarl_groot **out) {
  if (!out) return fail("groot_create: null argument");
  std::string err;
  if (gr_validate_create(d, err)) return fail("%s", err.c_str());
  aomarl_groot *g = new aomarl_groot();
  memset(g, 0, sizeof(*g));
  g->n_max = d->n_max; g->batch_max = d->batch_max; g->m_max = d->m_max; g->k_max = d->k_max;
  g->ldt = (d->k_max + 3) & ~3;
  const size_t big = (size_t)(d->k_max > d->m_max ? d->k_max : d->m_max);
  g->ws_floats = (size_t)GR_MAX_SPLIT * d->m_max * big;
  const size_t ntap = (size_t)d->batch_max * GR_MAX_TAPS, tab = GR_NTAB * sizeof(double);
  bool ok = hipMalloc((void **)&g->tabx, tab) == hipSuccess && hipMalloc((void **)&g->taby, tab) == hipSuccess &&
            hipMalloc((void **)&g->taps, ntap * sizeof(GrTap)) == hipSuccess &&
            hipHostMalloc((void **)&g->taps_host, ntap * sizeof(GrTap), hipHostMallocDefault) == hipSuccess &&
            hipEventCreateWithFlags(&g->staged, hipEventDisableTiming) == hipSuccess &&
            hipMemcpy(g->tabx, d->tabx, tab, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(g->taby, d->taby, tab, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && d->m_max > 0)
    ok = hipMalloc((void **)&g->T, (size_t)d->m_max * g->ldt * sizeof(float)) == hipSuccess &&
         hipMalloc((void **)&g->ws, g->ws_floats * sizeof(float)) == hipSuccess;
  ok = ok && hipEventRecord(g->staged, 0) == hipSuccess;
  if (!ok) {
    aomarl_groot_destroy(g);
    return fail("groot_create: device allocation failed (%d points, batch %d, sandwich %d x %d)", d->n_max, d->batch_max,
                d->m_max, d->k_max);
  }
  *out = g;
  return 0;
}

int aomarl_groot_form(aomarl_groot *g, const aomarl_groot_form_desc *f, const double *px, const double *py, int n,
                      float *out, int ldo, long long stride_o, void *stream) {
  if (!g) return fail("groot_form: null object");
  if (!px || !py || !out) return fail("groot_form: null px / py / out");
  std::string err;
  if (gr_validate_form(f, n, ldo, stride_o, g->n_max, g->batch_max, err)) return fail("%s", err.c_str());
  const int ntaps = gr_taps_per_entry(f);
  if (ntaps > GR_MAX_TAPS) return fail("groot_form: %d taps per entry, at most %d", ntaps, GR_MAX_TAPS);
  std::vector<GrTap> taps;
  gr_build_taps(f, taps);
  hipStream_t s = (hipStream_t)stream;
  // the object's previous call, on whatever stream it ran, has read both tap buffers: calls on different streams do
  // not race on them (they are serialised here instead)
  HIPCHK(hipEventSynchronize(g->staged));
  memcpy(g->taps_host, taps.data(), taps.size() * sizeof(GrTap));
  HIPCHK(hipMemcpyAsync(g->taps, g->taps_host, taps.size() * sizeof(GrTap), hipMemcpyHostToDevice, s));
  const unsigned tiles = (unsigned)((n + GR_TILE - 1) / GR_TILE);
  k_groot_form<<<dim3(tiles, tiles, (unsigned)f->batch), dim3(GR_TILE, GR_TILE), 0, s>>>(px, py, n, g->taps, ntaps, g->tabx,
                                                                                        g->taby, out, ldo, stride_o);
  LAUNCHCHK();
  HIPCHK(hipEventRecord(g->staged, s));
  return 0;
}

// C [M][ldc] (+)= A [M][K] . B [N][K]^T, slabs summed in order
static int gr_product(aomarl_groot *g, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C,
                      int ldc, int add, hipStream_t s) {
  const GemmPCfg c = gemm_p_pick(M, N, K, g->ws_floats, GR_MAX_SPLIT);
  if (c.wm == 0) return fail("groot_sandwich: no configuration of the matrix kernel for %d x %d x %d", M, N, K);
  if (!gemm_p_launch_cfg(c, M, N, K, 1.f, A, lda, B, ldb, add ? 1.f : 0.f, C, ldc, g->ws, 1, s))
    return fail("groot_sandwich: the matrix kernel could not be launched (tile %d x %d)", c.wm, c.wn);
  LAUNCHCHK();
  g_arith[AR_GEMM_F32]++;
  if (c.nz > 1) {
    const long long tot = (long long)M * N;
    k_groot_reduce<<<(unsigned)((tot + 255) / 256), 256, 0, s>>>(M, N, c.nz, g->ws, C, ldc, add);
    LAUNCHCHK();
  }
  return 0;
}

int aomarl_groot_sandwich(aomarl_groot *g, const float *G, int ldg, int m, const float *C, int ldc, int n, float *out,
                          int ldo, int accumulate, void *stream) {
  if (!g) return fail("groot_sandwich: null object");
  std::string err;
  if (gr_validate_sandwich(m, n, ldg, ldc, ldo, G, C, out, g->m_max, g->k_max, err)) return fail("%s", err.c_str());
  hipStream_t s = (hipStream_t)stream;
  if (gr_product(g, m, n, n, G, ldg, C, ldc, g->T, g->ldt, 0, s)) return 1;          // T = G C^T
  return gr_product(g, m, m, n, G, ldg, g->T, g->ldt, out, ldo, accumulate, s);      // out = G T^T
}
