// aomarl_mcao.hip -- multi-conjugate AO: mirrors conjugated to altitude (include/aomarl.h: aomarl_mcao_*).  gfx950 only.
// The model is ao_marl_amd/mcao.py (mirror_shape_model, mirrors_add_model, delay_line_model; float64 NumPy).  A
// translation unit of its own, like aomarl_tomo.hip: the calls read the context's delay, grids and pupils through
// aomarl_env_host.h, and hand the science field its mirrors through the same header.  The host half is aomarl_mcao_host.h.
#include "aomarl_env_host.h"
#include "aomarl_step_plan_host.h"      // delay_weights
#include "aomarl_field_host.h"          // FieldMirArgs
#include "aomarl_mcao_host.h"
#include "aomarl_mcao_sample.h"

struct McaoMirror {
  int dim, pitch, i1min, j1min, gw, gh, ss, nact, com_off;
  const int32_t *grid;     // [gh][gw]
  const float *prof;       // [ss]
};
struct McaoDev {
  int nmirrors, nact_total, plane_stride;      // plane_stride = dim_max^2: mirror m of environment e at (e M + m) stride
  McaoMirror mir[AOMARL_MCAO_MAX_MIRRORS];
};

struct aomarl_mcao {
  int nenv = 0;
  McaoDev dev = {};
  McaoPlan plan = {};
  int dims[AOMARL_MCAO_MAX_MIRRORS] = {0, 0};
  float *com = nullptr, *com1 = nullptr, *com2 = nullptr, *voltage = nullptr;      // [nenv][nact_total]
  float *planes = nullptr;                                                         // [nenv][M][dim_max^2]
  int32_t *grid[AOMARL_MCAO_MAX_MIRRORS] = {nullptr, nullptr};
  float *prof[AOMARL_MCAO_MAX_MIRRORS] = {nullptr, nullptr};
};

// =============================================================================================
// k_mcao_apply: the delay line of the altitude mirrors, k_delay's statement on the object's buffers.  It is compiled as
// k_delay is (the compiler's default contraction, nothing in front of it in this file changes it): the same expression
// under the same rules, so that a mirror driven with the simulator's commands carries the simulator's voltages to the bit.
// =============================================================================================
__global__ __launch_bounds__(256) void k_mcao_apply(float *__restrict__ com, float *__restrict__ com1, float *__restrict__ com2,
                                                    float *__restrict__ voltage, int nact, float a, float b, float c,
                                                    int env_begin) {
  const int e = env_begin + blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nact) return;
  const long long o = (long long)e * nact + i;
  const float c0 = com[o];
  const float c1 = com1[o], c2 = com2[o];
  voltage[o] = a * c0 + b * c1 + c * c2;
  com2[o] = c1;
  com1[o] = c0;
}

// Everything below is compiled without floating-point contraction, every fused multiply-add written as one, as
// aomarl_field.hip is: k_mcao_add exists in four instantiations and a direction must come out with the same bits from each.
#pragma clang fp contract(off)

// =============================================================================================
// k_mcao_shape: k_dm_shape_sep's idea on the object's mirrors.  One workgroup per 32 x 32 tile of a mirror's plane (the
// block index walks mirror 0's tiles, then mirror 1's: McaoPlan); the profile and the 12 x 12 lattice cells that can reach
// the tile are staged in LDS (a cell outside the lattice or without an actuator holds 0); a thread owns one column of the
// tile and four of its rows:
//     shape[y][x] = sum_gy u(y - Y_gy) (sum_gx u(x - X_gx) C[gy][gx]),   gx, gy ascending,
// every product a fused multiply-add onto the running sum.  No atomics; nothing depends on the launch.
// volts: [env_count][ldv] rows relative to env_begin.
// =============================================================================================
__global__ __launch_bounds__(MCAO_THREADS) void k_mcao_shape(McaoDev md, McaoPlan plan, const float *__restrict__ volts,
                                                             int ldv, float *__restrict__ planes, int env_begin) {
  __shared__ float sC[MCAO_CELLS][MCAO_CELLS + 1];
  __shared__ float sU[MCAO_MAX_SS];
  const int m = (plan.nmirrors > 1 && (int)blockIdx.x >= plan.first[1]) ? 1 : 0;
  const McaoMirror &D = md.mir[m];
  const int t = blockIdx.x - plan.first[m];
  const int ty = t / plan.tx[m], tx = t - ty * plan.tx[m];
  const int e = env_begin + blockIdx.y;
  const float *com = volts + (long long)blockIdx.y * ldv + D.com_off;
  float *shape = planes + ((long long)e * md.nmirrors + m) * md.plane_stride;
  const int tid = threadIdx.x;
  const int x0 = tx * MCAO_TILE, y0 = ty * MCAO_TILE;
  const int ss = D.ss, pitch = D.pitch;
  // the first lattice column / row whose patch can touch the tile: X_g + ss - 1 >= x0
  auto first_cell = [&](int p0, int pmin) {
    const int num = p0 - pmin - (ss - 1);
    return num >= 0 ? (num + pitch - 1) / pitch : -((-num) / pitch);
  };
  const int gxb = first_cell(x0, D.i1min), gyb = first_cell(y0, D.j1min);
  if (tid < ss) sU[tid] = D.prof[tid];
  if (tid < MCAO_CELLS * MCAO_CELLS) {
    const int r = tid / MCAO_CELLS, cc = tid - r * MCAO_CELLS;
    const int gx = gxb + cc, gy = gyb + r;
    float v = 0.f;
    if (gx >= 0 && gx < D.gw && gy >= 0 && gy < D.gh) {
      const int a = D.grid[gy * D.gw + gx];
      if (a >= 0) v = com[a];
    }
    sC[r][cc] = v;
  }
  __syncthreads();
  const int x = x0 + (tid & (MCAO_TILE - 1));
  float rs[MCAO_CELLS];
#pragma unroll
  for (int r = 0; r < MCAO_CELLS; r++) rs[r] = 0.f;
#pragma unroll
  for (int cc = 0; cc < MCAO_CELLS; cc++) {
    const int a = x - (D.i1min + pitch * (gxb + cc));
    const float wx = (a >= 0 && a < ss) ? sU[a] : 0.f;
#pragma unroll
    for (int r = 0; r < MCAO_CELLS; r++) rs[r] = __builtin_fmaf(wx, sC[r][cc], rs[r]);
  }
  if (x >= D.dim) return;
#pragma unroll
  for (int j = 0; j < MCAO_TILE / 8; j++) {
    const int y = y0 + (tid >> 5) + 8 * j;
    if (y >= D.dim) continue;
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < MCAO_CELLS; r++) {
      const int a = y - (D.j1min + pitch * (gyb + r));
      const float wy = (a >= 0 && a < ss) ? sU[a] : 0.f;
      acc = __builtin_fmaf(wy, rs[r], acc);
    }
    shape[y * D.dim + x] = acc;
  }
}

// =============================================================================================
// k_mcao_add<KT>: k_tomo_trace's shape.  A workgroup owns 256 consecutive pixels of the looking grid (side nn), a thread one
// pixel of all K planes of an environment.  The mirror loop is outside, the direction loop inside, the sums in KT named
// registers (KT is a template argument: the loops unroll); off and dm1 ride in the kernel's arguments.  A call of K
// directions runs the instantiation with the next power of two KT >= K; the slots past K have zero offsets (a read inside
// the plane or none at all) and are never loaded or stored.  Per direction the operations and their order do not depend on
// K, KT or the other directions.
// =============================================================================================
template <int KT>
__global__ __launch_bounds__(256) void k_mcao_add(McaoDev md, McaoAddArgs a, int K, const float *__restrict__ mplanes,
                                                  float *__restrict__ planes, const float *__restrict__ pupil, int nn,
                                                  int env_begin) {
  const int e = env_begin + blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nn * nn) return;
  const int y = p / nn, x = p - y * nn;
  float *out = planes + (long long)e * K * nn * nn + p;          // plane k of the environment: out[k nn nn]
  float v[KT];
#pragma unroll
  for (int k = 0; k < KT; k++) v[k] = k < K ? out[(long long)k * nn * nn] : 0.f;
  const float c = 0.5f * (float)(nn - 1);
  const float dx = (float)x - c, dy = (float)y - c;              // exact: half-integers below 2^23
#pragma unroll
  for (int m = 0; m < AOMARL_MCAO_MAX_MIRRORS; m++)
    if (m < md.nmirrors) {
      const float *pl = mplanes + ((long long)e * md.nmirrors + m) * md.plane_stride;
      const int dim = md.mir[m].dim;
#pragma unroll
      for (int k = 0; k < KT; k++)
        v[k] += mcao_bilinear(pl, dim, __builtin_fmaf(a.dm1[m][k], dx, (float)x + a.ox[m][k]),
                              __builtin_fmaf(a.dm1[m][k], dy, (float)y + a.oy[m][k]));
    }
#pragma unroll
  for (int k = 0; k < KT; k++)
    if (k < K) out[(long long)k * nn * nn] = pupil ? v[k] * pupil[p] : v[k];
}

// ------------------------------------------------------------------------------------------------- host side
int aomarl_mcao_destroy(aomarl_mcao *m) {
  if (!m) return 0;
  for (float *p : {m->com, m->com1, m->com2, m->voltage, m->planes, m->prof[0], m->prof[1]})
    if (p) (void)hipFree(p);
  for (int32_t *p : {m->grid[0], m->grid[1]})
    if (p) (void)hipFree(p);
  delete m;
  return 0;
}

int aomarl_mcao_create(aomarl_ctx *c, int nenv, const aomarl_mcao_desc *d, aomarl_mcao **out) {
  if (!c) return fail("mcao_create: null ctx");
  std::string err;
  if (mcao_validate_desc(d, nenv, out, err)) return fail("%s", err.c_str());
  aomarl_mcao *m = new aomarl_mcao();
  m->nenv = nenv;
  m->dev.nmirrors = d->nmirrors;
  int dmax = 0, coff = 0;
  bool ok = true;
  for (int k = 0; k < d->nmirrors && ok; k++) {
    const aomarl_mcao_mirror &M = d->mirrors[k];
    McaoMirror &D = m->dev.mir[k];
    D.dim = M.dim; D.pitch = M.pitch; D.i1min = M.i1min; D.j1min = M.j1min; D.gw = M.gw; D.gh = M.gh; D.ss = M.ss;
    D.nact = M.nact; D.com_off = coff;
    coff += M.nact;
    dmax = M.dim > dmax ? M.dim : dmax;
    m->dims[k] = M.dim;
    const size_t gb = (size_t)M.gw * M.gh * sizeof(int32_t), pb = (size_t)M.ss * sizeof(float);
    ok = hipMalloc((void **)&m->grid[k], gb) == hipSuccess && hipMalloc((void **)&m->prof[k], pb) == hipSuccess &&
         hipMemcpy(m->grid[k], M.grid, gb, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(m->prof[k], M.prof, pb, hipMemcpyHostToDevice) == hipSuccess;
    D.grid = m->grid[k]; D.prof = m->prof[k];
  }
  m->dev.nact_total = coff;
  m->dev.plane_stride = dmax * dmax;
  m->plan = mcao_plan(m->dims, d->nmirrors);
  const size_t nc = (size_t)nenv * coff, np = (size_t)nenv * d->nmirrors * m->dev.plane_stride;
  struct { float **p; size_t n; } bufs[5] = {{&m->com, nc}, {&m->com1, nc}, {&m->com2, nc}, {&m->voltage, nc}, {&m->planes, np}};
  for (auto &b : bufs)
    ok = ok && hipMalloc((void **)b.p, b.n * sizeof(float)) == hipSuccess && hipMemset(*b.p, 0, b.n * sizeof(float)) == hipSuccess;
  if (!ok) {
    aomarl_mcao_destroy(m);
    return fail("mcao_create: allocating %zu floats failed", 4 * nc + np);
  }
  HIPCHK(hipDeviceSynchronize());
  *out = m;
  return 0;
}

int aomarl_mcao_com(aomarl_mcao *m, float **com, float **voltage, float **planes) {
  if (!m) return fail("mcao_com: null object");
  if (com) *com = m->com;
  if (voltage) *voltage = m->voltage;
  if (planes) *planes = m->planes;
  return 0;
}

int aomarl_mcao_apply(aomarl_mcao *m, aomarl_ctx *c, int b, int n, const float *volts, void *stream) {
  if (!m || !c) return fail("mcao_apply: null argument");
  int rc = env_refuse_busy("mcao_apply", c);
  if (rc) return rc;
  std::string err;
  if (mcao_validate_range("mcao_apply", m->nenv, b, n, err)) return fail("%s", err.c_str());
  hipStream_t s = (hipStream_t)stream;
  const int na = m->dev.nact_total;
  if (!volts) {
    const DelayWeights dw = delay_weights(env_view(c).delay, false);
    hipLaunchKernelGGL(k_mcao_apply, dim3((na + 255) / 256, n), dim3(256), 0, s, m->com, m->com1, m->com2, m->voltage, na, dw.wa,
                       dw.wb, dw.wc, b);
    LAUNCHCHK();
    volts = m->voltage + (size_t)b * na;
  }
  hipLaunchKernelGGL(k_mcao_shape, dim3(m->plan.first[m->dev.nmirrors], n), dim3(MCAO_THREADS), 0, s, m->dev, m->plan, volts, na,
                     m->planes, b);
  LAUNCHCHK();
  return 0;
}

int aomarl_mcao_reset(aomarl_mcao *m, int b, int n, void *stream) {
  if (!m) return fail("mcao_reset: null object");
  std::string err;
  if (mcao_validate_range("mcao_reset", m->nenv, b, n, err)) return fail("%s", err.c_str());
  hipStream_t s = (hipStream_t)stream;
  const size_t na = m->dev.nact_total, ps = (size_t)m->dev.nmirrors * m->dev.plane_stride;
  for (float *p : {m->com, m->com1, m->com2, m->voltage}) HIPCHK(hipMemsetAsync(p + b * na, 0, n * na * sizeof(float), s));
  HIPCHK(hipMemsetAsync(m->planes + b * ps, 0, n * ps * sizeof(float), s));
  return 0;
}

int aomarl_mcao_add(aomarl_mcao *m, aomarl_ctx *c, const aomarl_mcao_view *v, float *planes, int ndir, int nn, int b, int n,
                    int flags, void *stream) {
  if (!m || !c) return fail("mcao_add: null argument");
  int rc = env_refuse_busy("mcao_add", c);
  if (rc) return rc;
  const EnvView ev = env_view(c);
  std::string err;
  if (mcao_validate_add(v, planes, ndir, nn, ev.sys.n, ev.sys.pupdiam, m->dev.nmirrors, m->dims, m->nenv, b, n, flags,
                        AOMARL_TRACE_MASK, err))
    return fail("%s", err.c_str());
  const McaoAddArgs a = mcao_add_args(v, m->dev.nmirrors);
  // (n == pupdiam: the sensor's grid is the pupil grid's size and its pupil is asked for first, as aomarl_tomo_trace's)
  const float *pupil = !(flags & AOMARL_TRACE_MASK) ? nullptr : nn == ev.sys.n ? ev.sys.mpupil : ev.sys.spupil;
  const int np = nn * nn;
#define MCAO_ADD(KT)                                                                                                          \
  hipLaunchKernelGGL(k_mcao_add<KT>, dim3((np + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, m->dev, a, ndir, m->planes, \
                     planes, pupil, nn, b)
  switch (mcao_slots(ndir)) {
    case 1: MCAO_ADD(1); break;
    case 2: MCAO_ADD(2); break;
    case 4: MCAO_ADD(4); break;
    default: MCAO_ADD(8); break;
  }
#undef MCAO_ADD
  LAUNCHCHK();
  return 0;
}

// ---- the science field through the mirrors (the field's kernels: aomarl_field.hip, field_pixel<KT, true>)
int aomarl_field_attach_mirrors(aomarl_field *f, aomarl_mcao *m, const aomarl_mcao_view *v) {
  if (!f || !m) return fail("field_attach_mirrors: null argument");
  int fnenv, fndir, fpd;
  field_dims(f, &fnenv, &fndir, &fpd);
  if (fnenv != m->nenv) return fail("field_attach_mirrors: the field has %d environments, the mirrors %d", fnenv, m->nenv);
  std::string err;
  if (mcao_validate_attach(v, fndir, m->dev.nmirrors, m->dims, fpd, err)) return fail("%s", err.c_str());
  FieldMirArgs base;
  memset(&base, 0, sizeof(base));
  base.planes = m->planes;
  base.nmirrors = m->dev.nmirrors;
  base.stride = m->dev.plane_stride;
  for (int k = 0; k < m->dev.nmirrors; k++) base.dim[k] = m->dims[k];
  field_set_mirrors(f, m, base, v->off);
  return 0;
}

int aomarl_field_detach_mirrors(aomarl_field *f) {
  if (!f) return fail("field_detach_mirrors: null object");
  field_clear_mirrors(f);
  return 0;
}
