// aomarl_capi_dmreg.hip -- mirror mis-registration per environment (include/aomarl.h: aomarl_dmreg_*; reference:
// dmCompass.py:148-176).  A translation unit of its own: the trace reads the context's static description and the state
// exactly as aomarl_raytrace_wfs / _target do, through aomarl_env_host.h.  The host half is aomarl_dmreg_host.h.
#include "aomarl_env_host.h"
#include "aomarl_trace_dev.h"
#include "aomarl_dmreg_host.h"

// =============================================================================================
// k_trace_reg: k_raytrace with every mirror sampled through its affine row.
//
// Shape.  k_raytrace's own: a workgroup of 256 threads owns 256 consecutive pixels of the grid, a wave 64 of them.  A
// workgroup's store is 1 KiB of contiguous memory -- eight whole 128-byte lines -- whatever nn is, and the workgroups in
// flight at one time cover one contiguous stretch of every buffer, which is what the memory's open pages want.  For the
// rotations users set (|A01| 64 < 1 up to a degree) the four gathers of a wave walk at most two rows of a plane over a
// contiguous run of ~65 floats (twice that where the wave crosses the end of a grid row): 3 lines a row.  Two other
// shapes were built and measured at 40x40 / 256 environments: tiles of 64 x 4 pixels, and waves that walk
// a whole grid row with the layers' row arithmetic in scalar registers.  Both keep the vertical neighbours in one
// CU's vector cache and both lost, by 2 to 20 %: their partial tiles and last steps cost a full trip to memory for a
// few lanes (nn = 644 = 10 x 64 + 4), and their workgroups in flight are spread over many rows.  The footprint is not
// staged in LDS: nothing here is short of cache hits.
//
// Uniform data.  The six numbers of an (environment, mirror) pair are the same for every lane: the address depends on
// blockIdx and the arguments alone, the table is const and restrict, and the loads are scalar loads into scalar
// registers, once per wave through the scalar cache -- no lane loads them and no barrier holds a workgroup back (a
// version that staged them in LDS once per workgroup put a trip to memory and a barrier in front of every workgroup's
// first load).
//
// One pass: layers and mirrors are summed in a register in k_raytrace's order, one store per pixel; the buffer is read
// only without AOMARL_TRACE_RESET.  The arithmetic per pixel is k_raytrace's, expression for expression.
// =============================================================================================
#define TREG_THREADS 256
// bilinear_ring with the mirrors' whole-pixel shortcut: where both weights are zero -- every layer of an on-axis system
// -- bilinear_ring's expression is v00 + 0 v01 + 0 (...), the value of the floor cell, and its three other loads, four
// ring addresses and seven products are spent on zeros.  The trace is bound by vector instructions, and
// these are most of them.  (The two differ where a screen holds an infinity, and in the sign of a zero.)
__device__ __forceinline__ float bilinear_ring_cell(const float *in, int N, int ox, int oy, float fx, float fy) {
  int ix = (int)floorf(fx), iy = (int)floorf(fy);
  float wx = fx - (float)ix, wy = fy - (float)iy;
  if (ix < 0 || iy < 0 || ix >= N || iy >= N) return 0.f;
  float v00 = in[ring_idx(ix, iy, ox, oy, N)];
  if (wx == 0.f && wy == 0.f) return v00;
  int ix1 = ix + 1 < N ? ix + 1 : ix, iy1 = iy + 1 < N ? iy + 1 : iy;
  float v01 = in[ring_idx(ix1, iy, ox, oy, N)];
  float v10 = in[ring_idx(ix, iy1, ox, oy, N)], v11 = in[ring_idx(ix1, iy1, ox, oy, N)];
  return (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
}
template <bool TARGET>
__global__ __launch_bounds__(TREG_THREADS) void k_trace_reg(DevSys sys, DevState st, const float *__restrict__ table,
                                                            int env_begin, int flags) {
  const int nn = TARGET ? sys.pupdiam : sys.n;
  const int e = env_begin + blockIdx.y;
  float *out = (TARGET ? st.tar_phase : st.wfs_phase) + (long long)e * nn * nn;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nn * nn) return;
  const int y = p / nn, x = p - y * nn;
  float v = (flags & AOMARL_TRACE_RESET) ? 0.f : out[p];
  if (flags & AOMARL_TRACE_ATMOS) {
    for (int l = 0; l < sys.nlayers; l++) {
      const DevLayer &L = sys.layers[l];
      const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
      const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
      v += bilinear_ring_cell(base, L.dim, ox, oy, (float)x + (TARGET ? L.txo : L.wxo),
                              (float)y + (TARGET ? L.tyo : L.wyo));
    }
  }
  if (flags & AOMARL_TRACE_DMS) {
    const float *__restrict__ rows = table + (long long)e * sys.ndm * DMREG_ROW;
    const float c = 0.5f * (float)(nn - 1);
    const float dx = (float)x - c, dy = (float)y - c;      // exact: half-integers below 2^23
    for (int k = 0; k < sys.ndm; k++) {
      const DevDm &D = sys.dms[k];
      const float *__restrict__ r = rows + k * DMREG_ROW;  // uniform: scalar loads
      // (aomarl_dmreg_host.h: dmreg_sample) the identity row gives (x + ox, y + oy) exactly
      const float fx = (c + (TARGET ? D.txo : D.wxo)) + (r[0] * dx + (r[1] * dy + r[4]));
      const float fy = (c + (TARGET ? D.tyo : D.wyo)) + (r[2] * dx + (r[3] * dy + r[5]));
      const int ix = (int)floorf(fx), iy = (int)floorf(fy);
      if (ix >= 0 && iy >= 0 && ix < D.dim && iy < D.dim) {
        const float wx = fx - (float)ix, wy = fy - (float)iy;
        const int ix1 = ix + 1 < D.dim ? ix + 1 : ix, iy1 = iy + 1 < D.dim ? iy + 1 : iy;
        float v00 = dm_value(sys, st, e, k, ix, iy);
        if (wx == 0.f && wy == 0.f) {
          v += v00;
        } else {
          float v01 = dm_value(sys, st, e, k, ix1, iy), v10 = dm_value(sys, st, e, k, ix, iy1);
          float v11 = dm_value(sys, st, e, k, ix1, iy1);
          v += (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
        }
      }
    }
  }
  if (flags & AOMARL_TRACE_MASK) v *= (TARGET ? sys.spupil : sys.mpupil)[p];
  out[p] = v;
}

struct aomarl_dmreg {
  const aomarl_ctx *owner = nullptr;
  int nenv = 0, ndm = 0;
  int dim[AOMARL_MAX_DMS];
  float *table = nullptr;          // device [nenv][ndm][6]
};

// dmreg_validate_ctx on a context's busy bits: this unit's own wording of the two refusals
static int dmreg_refuse_busy(const aomarl_ctx *c, const char *who, std::string &err) {
  const int busy = env_busy(c);
  return dmreg_validate_ctx(busy & ENV_PIPELINED, busy & ENV_RESET_PREFETCHED, who, err);
}

int aomarl_dmreg_destroy(aomarl_dmreg *r) {
  if (!r) return 0;
  if (r->table) { (void)hipDeviceSynchronize(); (void)hipFree(r->table); }
  delete r;
  return 0;
}

int aomarl_dmreg_create(aomarl_ctx *c, int nenv, aomarl_dmreg **out) {
  if (!c || !out) return fail("dmreg_create: null argument");
  *out = nullptr;
  std::string err;
  const EnvView v = env_view(c);
  if (dmreg_validate_create(nenv, v.ndm, err)) return fail("%s", err.c_str());
  if (dmreg_refuse_busy(c, "dmreg_create", err)) return fail("%s", err.c_str());
  for (int k = 0; k < v.ndm; k++) {
    const DevDm &D = v.sys.dms[k];
    if (dmreg_validate_geometry(v.sys.n, D.wxo, D.wyo, D.dim, k, err) ||
        dmreg_validate_geometry(v.sys.pupdiam, D.txo, D.tyo, D.dim, k, err))
      return fail("%s", err.c_str());
  }
  aomarl_dmreg *r = new aomarl_dmreg();
  r->owner = c; r->nenv = nenv; r->ndm = v.ndm;
  for (int k = 0; k < v.ndm; k++) r->dim[k] = v.sys.dms[k].dim;
  const size_t rows = (size_t)nenv * (size_t)v.ndm;
  std::vector<float> ident(rows * DMREG_ROW);
  dmreg_identity(ident.data(), (long long)rows);
  hipError_t e = hipMalloc((void **)&r->table, sizeof(float) * rows * DMREG_ROW);
  if (e == hipSuccess) e = hipMemcpy(r->table, ident.data(), sizeof(float) * rows * DMREG_ROW, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    aomarl_dmreg_destroy(r);
    return fail("dmreg_create: %s", hipGetErrorString(e));
  }
  *out = r;
  return 0;
}

int aomarl_dmreg_set(aomarl_dmreg *r, int b, int n, int dm, const float *At, void *stream) {
  if (!r) return fail("dmreg_set: null object");
  std::string err;
  if (dmreg_validate_range(r->nenv, r->ndm, b, n, dm, "dmreg_set", err)) return fail("%s", err.c_str());
  if (dmreg_validate_rows(At, n, r->dim[dm], err)) return fail("%s", err.c_str());
  hipStream_t s = (hipStream_t)stream;
  // rows of one mirror are DMREG_ROW floats every ndm rows: a strided copy from the caller's array, complete (for
  // this pageable source) when the call returns, ordered on the stream behind the kernels that read the old rows
  HIPCHK(hipMemcpy2DAsync(r->table + ((size_t)b * r->ndm + dm) * DMREG_ROW, sizeof(float) * DMREG_ROW * r->ndm, At,
                          sizeof(float) * DMREG_ROW, sizeof(float) * DMREG_ROW, (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int aomarl_dmreg_get(aomarl_dmreg *r, int b, int n, int dm, float *At, void *stream) {
  if (!r || !At) return fail("dmreg_get: null argument");
  std::string err;
  if (dmreg_validate_range(r->nenv, r->ndm, b, n, dm, "dmreg_get", err)) return fail("%s", err.c_str());
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpy2DAsync(At, sizeof(float) * DMREG_ROW, r->table + ((size_t)b * r->ndm + dm) * DMREG_ROW,
                          sizeof(float) * DMREG_ROW * r->ndm, sizeof(float) * DMREG_ROW, (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int aomarl_dmreg_trace(aomarl_dmreg *r, aomarl_ctx *c, aomarl_state *st, int b, int n, int target, int flags, void *stream) {
  if (!r || !c || !st) return fail("dmreg_trace: null argument");
  if (r->owner != c) return fail("dmreg_trace: the table was created with another context");
  std::string err;
  if (dmreg_refuse_busy(c, "dmreg_trace", err)) return fail("%s", err.c_str());
  if (st->nenv != r->nenv) return fail("dmreg_trace: the table has %d environments, the state %d", r->nenv, st->nenv);
  const int known = AOMARL_TRACE_ATMOS | AOMARL_TRACE_DMS | AOMARL_TRACE_RESET | AOMARL_TRACE_MASK;
  if (dmreg_validate_trace(r->nenv, b, n, target, flags, known, err)) return fail("%s", err.c_str());
  const int rc = env_trace_ready(c, st, b, n, flags, stream);
  if (rc) return rc;
  if (!(target ? st->tar_phase : st->wfs_phase)) return fail("dmreg_trace needs st->%s", target ? "tar_phase" : "wfs_phase");
  if (n == 0) return 0;
  const EnvView v = env_view(c);
  const int nn = target ? v.sys.pupdiam : v.sys.n;
  const dim3 grid((nn * nn + TREG_THREADS - 1) / TREG_THREADS, n);
  if (target)
    hipLaunchKernelGGL(k_trace_reg<true>, grid, dim3(TREG_THREADS), 0, (hipStream_t)stream, v.sys, dev_state(st), r->table, b, flags);
  else
    hipLaunchKernelGGL(k_trace_reg<false>, grid, dim3(TREG_THREADS), 0, (hipStream_t)stream, v.sys, dev_state(st), r->table, b, flags);
  LAUNCHCHK();
  return 0;
}
