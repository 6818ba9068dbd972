// aomarl_field.hip -- the science field (include/aomarl.h: aomarl_field_*).  gfx950 only.
// The model is ao_marl_amd/field.py (field_trace_model, FieldModel; float64 NumPy).  A translation unit of its own, like
// aomarl_tomo.hip: the trace reads the context's static description and the state through aomarl_env_host.h, the PSF
// finish reuses psf_window_fit, fit_axis_gain and strehl_commit_body (aomarl_trace_dev.h) on the field's own buffers.  The
// host half is aomarl_field_host.h.
#include "aomarl_env_host.h"
#include "aomarl_stage_host.h"        // launch_strehl_reset, launch_strehl_fit_le (aomarl_target.hip) on the field's buffers
#include "aomarl_trace_dev.h"
#include "aomarl_field_host.h"
#include "aomarl_mcao_sample.h"

// Everything below is compiled without floating-point contraction: where a multiply-add is fused it is written as one
// (__builtin_fmaf).  The kernels exist in several instantiations (the direction count is a template argument) and a
// direction must come out with the same bits from each; left to the compiler, which products are fused with which sums
// differs between instantiations.  (The headers above come first: the helpers they define keep the default contraction.)
#pragma clang fp contract(off)

// bilinear_ring with the operations spelled out: zero outside the screen, the last line clamped; weights of zero give
// the floor cell's value exactly (1 v00 + 0 v01), so whole-pixel offsets have aomarl_raytrace_target's bits
__device__ __forceinline__ float field_bilinear(const float *in, int N, int ox, int oy, float fx, float fy) {
  const int ix = (int)floorf(fx), iy = (int)floorf(fy);
  const float wx = fx - (float)ix, wy = fy - (float)iy;
  if (ix < 0 || iy < 0 || ix >= N || iy >= N) return 0.f;
  const int ix1 = ix + 1 < N ? ix + 1 : ix, iy1 = iy + 1 < N ? iy + 1 : iy;
  const float v00 = in[ring_idx(ix, iy, ox, oy, N)], v01 = in[ring_idx(ix1, iy, ox, oy, N)];
  const float v10 = in[ring_idx(ix, iy1, ox, oy, N)], v11 = in[ring_idx(ix1, iy1, ox, oy, N)];
  const float top = __builtin_fmaf(wx, v01, (1.f - wx) * v00), bot = __builtin_fmaf(wx, v11, (1.f - wx) * v10);
  return __builtin_fmaf(wy, bot, (1.f - wy) * top);
}

struct aomarl_field {
  int nenv = 0, ndir = 0, nlayers = 0, W = 0, pd = 0, nblk = 0, chunk = 0;
  float inv_lambda = 0.f, ref_peak = 0.f;
  std::vector<float> off;              // HOST [ndir][nlayers][2]
  std::vector<FieldLaunch> plan;
  float *record = nullptr;             // [nenv][ndir][8]
  float *le = nullptr;                 // [nenv][ndir][W][W]
  float *TR = nullptr;                 // [nenv][chunk][pupdiam][W][2]: stage 1 of the launch's directions
  float *TPART = nullptr;              // [nenv][chunk][nblk][4]: (sum d, sum d^2, lit pixels, -) per row block
  float *PEND = nullptr;               // [nenv][ndir][W W + 4]: window, variance, fitted gain
  // mirrors at altitude (aomarl_field_attach_mirrors, aomarl_mcao.hip): the object whose planes the directions see, and
  // the directions' offsets on them, HOST [ndir][nmirrors][2]; null: none
  const struct aomarl_mcao *mir = nullptr;
  std::vector<float> mir_off;
  FieldMirArgs mir_base = {};          // planes, nmirrors, stride, dim of the attached object (no offsets)
};

// =============================================================================================
// The phase of pixel (x, y) of the pupil grid in the KT direction slots of the launch: the direction loop inside the layer
// loop (a layer's constants are read once, the directions' footprints overlap in the cache), the sums in KT named
// registers (KT is a template argument: the loops unroll, no branch and no run-time index into a register array), the
// offsets in the kernel's arguments (uniform: scalar registers).  A launch of K directions runs the instantiation with the
// next power of two KT >= K; the slots past K have zero offsets (a read inside the screens) and their sums are never
// stored.  Each mirror is evaluated once per pixel by the target's rule (trace_dm_values<true>: trace_dms<true>'s
// expression) and added to every direction in controller order, after the layers.  Per direction the operations and their
// order do not depend on K, KT or the other directions.  ALT: behind the pupil mirrors, the attached object's mirrors at
// altitude per direction, in mirror order, by k_mcao_add's sampling function (mcao_bilinear) with dm1 = 0; without ALT the
// text is what it was.
// =============================================================================================
template <int KT, bool ALT = false>
__device__ __forceinline__ void field_pixel(const DevSys &sys, const DevState &st, const FieldArgs &a, int e, int x, int y,
                                            int flags, float (&v)[KT],
                                            const typename FieldMir<ALT>::type &ma = typename FieldMir<ALT>::type()) {
  if (flags & AOMARL_TRACE_ATMOS) {
    for (int l = 0; l < sys.nlayers; l++) {
      const DevLayer &L = sys.layers[l];
      const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
      const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
#pragma unroll
      for (int k = 0; k < KT; k++) v[k] += field_bilinear(base, L.dim, ox, oy, (float)x + a.ox[l][k], (float)y + a.oy[l][k]);
    }
  }
  if (flags & AOMARL_TRACE_DMS) {
    float dmv[AOMARL_MAX_DMS];
    const unsigned has = trace_dm_values<true>(sys, st, e, x, y, dmv);
#pragma unroll
    for (int m = 0; m < AOMARL_MAX_DMS; m++)
      if (has & (1u << m)) {
#pragma unroll
        for (int k = 0; k < KT; k++) v[k] += dmv[m];
      }
  }
  if constexpr (ALT) {
    if (flags & AOMARL_TRACE_DMS) {
#pragma unroll
      for (int m = 0; m < FIELD_MAX_ALT; m++)
        if (m < ma.nmirrors) {
          const float *pl = ma.planes + ((long long)e * ma.nmirrors + m) * ma.stride;
#pragma unroll
          for (int k = 0; k < KT; k++) v[k] += mcao_bilinear(pl, ma.dim[m], (float)x + ma.ox[m][k], (float)y + ma.oy[m][k]);
        }
    }
  }
}

// =============================================================================================
// k_field_rows: k_target_rows for every direction of the launch -- trace, amplitude and the first DFT stage
//   R_k[y][kx] = sum_x a_k(y, x) exp(-2 pi i kx x / Npsf),  kx in [-hw, hw),
// in one launch; no phase plane goes to memory.  A workgroup owns RB = 256 / W pupil rows and walks them in chunks of W
// columns: a thread traces ONE pixel of the chunk in all directions (pupil, mirrors and the layers' constants read once),
// wraps each phase before the sincospif and leaves the amplitudes in LDS; then thread (row, kx) adds the chunk's W columns
// to its accumulators, two columns per 16-byte LDS read, the twiddle of a column read once for all directions (columns
// past the pupil grid hold zero amplitudes: they add nothing).  Variance sums per direction against the pivot -- the
// direction's own phase at the pupil grid's centre --, reduced over the workgroup by a tree in LDS: a fixed order.  All
// LDS is dynamic: [KT][256] float2 amplitudes (reused by the reduction) | [256] counts | [Npsf] float2 twiddles when
// Npsf <= FIELD_TW_LDS (at most 49 KiB with 16 directions).  W is even (2 hw).
// =============================================================================================
template <int KT, bool ALT>
__device__ __forceinline__ void field_rows_body(DevSys sys, DevState st, FieldArgs a, int K, int chunk, float inv_lambda,
                                                int env_begin, int flags, float *__restrict__ TR, float *__restrict__ TPART,
                                                int nblk, typename FieldMir<ALT>::type ma) {
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  const int W = 2 * sys.hw, RB = FIELD_THREADS / W, pd = sys.pupdiam, np = sys.npsf;
  float2 *samp = reinterpret_cast<float2 *>(fsm);                       // [KT][256]
  float *scnt = fsm + 2 * FIELD_THREADS * KT;                           // [256]
  float2 *stw = reinterpret_cast<float2 *>(scnt + FIELD_THREADS);       // [np]
  const bool tw_lds = np <= FIELD_TW_LDS;
  const int tid = threadIdx.x;
  const int e = env_begin + blockIdx.y;
  const int y0 = blockIdx.x * RB;
  const float2 *gtw = reinterpret_cast<const float2 *>(sys.psf_tw);
  if (tw_lds)
    for (int j = tid; j < np; j += FIELD_THREADS) stw[j] = gtw[j];
  const float2 *tw = tw_lds ? stw : gtw;
  float pivot[KT];
#pragma unroll
  for (int k = 0; k < KT; k++) pivot[k] = 0.f;
  field_pixel<KT, ALT>(sys, st, a, e, pd / 2, pd / 2, flags, pivot, ma);
  // the chunk's pixel of this thread, and its output element
  const int py = tid / W, px = tid - py * W;           // (py < RB: the threads past RB W idle in the trace)
  const int kxi = px, ys = py, kxf = kxi - sys.hw;
  float accr[KT], acci[KT], sd[KT], sd2[KT];
#pragma unroll
  for (int k = 0; k < KT; k++) accr[k] = acci[k] = sd[k] = sd2[k] = 0.f;
  float sm = 0.f;
  for (int x0 = 0; x0 < pd; x0 += W) {
    __syncthreads();
    {
      const int y = y0 + py, x = x0 + px;
      float m = 0.f;
      if (py < RB && y < pd && x < pd) m = sys.spupil[y * pd + x];
      float v[KT];
#pragma unroll
      for (int k = 0; k < KT; k++) v[k] = 0.f;
      if (m != 0.f) {
        field_pixel<KT, ALT>(sys, st, a, e, x, y, flags, v, ma);
        sm += 1.f;
      }
#pragma unroll
      for (int k = 0; k < KT; k++) {
        float2 amp = make_float2(0.f, 0.f);
        if (m != 0.f) {
          float t = v[k] * inv_lambda;
          t -= rintf(t);
          float sn, cs;
          sincospif(2.0f * t, &sn, &cs);
          amp = make_float2(m * cs, m * sn);
          const float d = v[k] - pivot[k];
          sd[k] += d; sd2[k] = __builtin_fmaf(d, d, sd2[k]);
        }
        samp[k * FIELD_THREADS + tid] = amp;
      }
    }
    __syncthreads();
    if (ys < RB) {
      // the chunk's W columns are summed from zero and then added to the row's sum: a blocked sum, whose round-off grows
      // with W + pd / W terms instead of pd
      float cr[KT], ci[KT];
#pragma unroll
      for (int k = 0; k < KT; k++) cr[k] = ci[k] = 0.f;
      for (int xx = 0; xx < W; xx += 2) {
        const float2 w0 = tw[(kxf * (x0 + xx)) & (np - 1)];        // (cos, sin); e^{-i t} = cos - i sin
        const float2 w1 = tw[(kxf * (x0 + xx + 1)) & (np - 1)];
#pragma unroll
        for (int k = 0; k < KT; k++) {
          const float4 am = *reinterpret_cast<const float4 *>(samp + k * FIELD_THREADS + ys * W + xx);   // columns xx, xx + 1
          cr[k] = __builtin_fmaf(am.y, w0.y, __builtin_fmaf(am.x, w0.x, cr[k]));
          ci[k] = __builtin_fmaf(-am.x, w0.y, __builtin_fmaf(am.y, w0.x, ci[k]));
          cr[k] = __builtin_fmaf(am.w, w1.y, __builtin_fmaf(am.z, w1.x, cr[k]));
          ci[k] = __builtin_fmaf(-am.z, w1.y, __builtin_fmaf(am.w, w1.x, ci[k]));
        }
      }
#pragma unroll
      for (int k = 0; k < KT; k++) { accr[k] += cr[k]; acci[k] += ci[k]; }
    }
  }
  if (ys < RB && y0 + ys < pd) {
#pragma unroll
    for (int k = 0; k < KT; k++)
      if (k < K) {
        float *o = TR + ((((long long)e * chunk + k) * pd + (y0 + ys)) * W + kxi) * 2;
        o[0] = accr[k]; o[1] = acci[k];
      }
  }
  // the workgroup's partial sums of the variance, per direction
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KT; k++) samp[k * FIELD_THREADS + tid] = make_float2(sd[k], sd2[k]);
  scnt[tid] = sm;
  __syncthreads();
  for (int o = FIELD_THREADS / 2; o >= 1; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < KT; k++) {
        const float2 p = samp[k * FIELD_THREADS + tid], q = samp[k * FIELD_THREADS + tid + o];
        samp[k * FIELD_THREADS + tid] = make_float2(p.x + q.x, p.y + q.y);
      }
      scnt[tid] += scnt[tid + o];
    }
    __syncthreads();
  }
  if (tid < K) {
    float *pp = TPART + ((((long long)e * chunk + tid) * nblk) + blockIdx.x) * 4;
    const float2 p = samp[tid * FIELD_THREADS];
    pp[0] = p.x; pp[1] = p.y; pp[2] = scnt[0]; pp[3] = 0.f;
  }
}

// the kernel as it was, and the one that sees mirrors at altitude (its FieldMirArgs behind the other arguments)
template <int KT>
__global__ __launch_bounds__(FIELD_THREADS) void k_field_rows(DevSys sys, DevState st, FieldArgs a, int K, int chunk,
                                                              float inv_lambda, int env_begin, int flags,
                                                              float *__restrict__ TR, float *__restrict__ TPART, int nblk) {
  field_rows_body<KT, false>(sys, st, a, K, chunk, inv_lambda, env_begin, flags, TR, TPART, nblk, FieldNoMirrors());
}
template <int KT>
__global__ __launch_bounds__(FIELD_THREADS) void k_field_rows_alt(DevSys sys, DevState st, FieldArgs a, int K, int chunk,
                                                                  float inv_lambda, int env_begin, int flags,
                                                                  float *__restrict__ TR, float *__restrict__ TPART, int nblk,
                                                                  FieldMirArgs ma) {
  field_rows_body<KT, true>(sys, st, a, K, chunk, inv_lambda, env_begin, flags, TR, TPART, nblk, ma);
}

// =============================================================================================
// k_field_finish: one workgroup per (direction of the launch, environment).  k_target_finish on the field's buffers --
// stage 2 G[ky][kx] = sum_y R[y][kx] exp(-2 pi i ky y / Npsf) in double, |G|^2 into the direction's pending window, the short
// exposure's fit (psf_window_fit), the variance from the row blocks' partials in their order -- and then, behind a
// barrier, k_strehl_commit's body on the field's record and long-exposure sum (a DevState whose strehl / le_img are the
// field's, "environment" e ndir + d).
// =============================================================================================
__global__ __launch_bounds__(256) void k_field_finish(DevSys sys, DevState fst, int ndir, int first, int chunk, int env_begin,
                                                      const float *__restrict__ TR, const float *__restrict__ TPART, int nblk,
                                                      float *__restrict__ PEND) {
  const int W = 2 * sys.hw, pd = sys.pupdiam, np = sys.npsf;
  const int k = blockIdx.x, e = env_begin + blockIdx.y;
  const int slot = e * ndir + first + k;
  const float2 *tw = reinterpret_cast<const float2 *>(sys.psf_tw);
  const float2 *R = reinterpret_cast<const float2 *>(TR) + ((long long)e * chunk + k) * pd * W;
  float *pend = PEND + (long long)slot * (W * W + 4);
  for (int o = threadIdx.x; o < W * W; o += blockDim.x) {
    const int ky = o / W, kx = o - ky * W;
    const int kyf = ky - sys.hw;
    double gr = 0., gi = 0.;                         // (pupdiam terms per element, one workgroup per direction: double is free here)
    for (int y = 0; y < pd; y++) {
      const float2 r = R[y * W + kx];
      const float2 w = tw[(kyf * y) & (np - 1)];
      gr = __builtin_fma((double)r.y, (double)w.y, __builtin_fma((double)r.x, (double)w.x, gr));
      gi = __builtin_fma(-(double)r.x, (double)w.y, __builtin_fma((double)r.y, (double)w.x, gi));
    }
    pend[o] = (float)__builtin_fma(gr, gr, gi * gi);
  }
  __syncthreads();
  psf_window_fit(pend, W);
  if (threadIdx.x == 0) {
    double sd = 0., sd2 = 0., sm = 0.;
    for (int b = 0; b < nblk; b++) {
      const float *pp = TPART + (((long long)e * chunk + k) * nblk + b) * 4;
      sd += pp[0]; sd2 += pp[1]; sm += pp[2];
    }
    double var = 0.;
    if (sm > 0.) { double mean = sd / sm; var = sd2 / sm - mean * mean; }
    pend[W * W] = (float)var;
  }
  __syncthreads();
  strehl_commit_body(sys, fst, 0, slot, PEND);
}

// the traced planes alone (tests, users of the off-axis phase): k_tomo_trace's shape on the pupil grid
template <int KT, bool ALT>
__device__ __forceinline__ void field_trace_body(DevSys sys, DevState st, FieldArgs a, int K, int ndir, int first,
                                                 float *__restrict__ planes, int env_begin, int flags,
                                                 typename FieldMir<ALT>::type ma) {
  const int pd = sys.pupdiam;
  const int e = env_begin + blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pd * pd) return;
  const int y = p / pd, x = p - y * pd;
  float *out = planes + ((long long)e * ndir + first) * pd * pd + p;          // plane k of the launch: out[k pd pd]
  float v[KT];
#pragma unroll
  for (int k = 0; k < KT; k++) v[k] = (k < K && !(flags & AOMARL_TRACE_RESET)) ? out[(long long)k * pd * pd] : 0.f;
  field_pixel<KT, ALT>(sys, st, a, e, x, y, flags, v, ma);
  const float mk = (flags & AOMARL_TRACE_MASK) ? sys.spupil[p] : 1.f;
#pragma unroll
  for (int k = 0; k < KT; k++)
    if (k < K) out[(long long)k * pd * pd] = (flags & AOMARL_TRACE_MASK) ? v[k] * mk : v[k];
}

template <int KT>
__global__ __launch_bounds__(256) void k_field_trace(DevSys sys, DevState st, FieldArgs a, int K, int ndir, int first,
                                                     float *__restrict__ planes, int env_begin, int flags) {
  field_trace_body<KT, false>(sys, st, a, K, ndir, first, planes, env_begin, flags, FieldNoMirrors());
}
template <int KT>
__global__ __launch_bounds__(256) void k_field_trace_alt(DevSys sys, DevState st, FieldArgs a, int K, int ndir, int first,
                                                         float *__restrict__ planes, int env_begin, int flags, FieldMirArgs ma) {
  field_trace_body<KT, true>(sys, st, a, K, ndir, first, planes, env_begin, flags, ma);
}

// the instantiation of a launch of K directions: the next power of two
#define FIELD_DISPATCH(K, CALL)                              \
  do {                                                       \
    if ((K) <= 1) { CALL(1); }                               \
    else if ((K) <= 2) { CALL(2); }                          \
    else if ((K) <= 4) { CALL(4); }                          \
    else if ((K) <= 8) { CALL(8); }                          \
    else { CALL(16); }                                       \
  } while (0)
static_assert(AOMARL_FIELD_MAX_DIRS == 16, "FIELD_DISPATCH covers 1..16 directions");

// ------------------------------------------------------------------------------------------------- host side
static FieldSys field_sys(const EnvView &v) {
  FieldSys sy;
  memset(&sy, 0, sizeof(sy));
  sy.nlayers = v.nlayers; sy.pupdiam = v.sys.pupdiam; sy.hw = v.sys.hw; sy.ndm = v.ndm;
  for (int l = 0; l < v.nlayers; l++) sy.dims[l] = v.sys.layers[l].dim;
  for (int k = 0; k < v.ndm; k++) { sy.dm_dim[k] = v.sys.dms[k].dim; sy.dm_txo[k] = v.sys.dms[k].txo; sy.dm_tyo[k] = v.sys.dms[k].tyo; }
  return sy;
}

int aomarl_field_destroy(aomarl_field *f) {
  if (!f) return 0;
  for (float *p : {f->record, f->le, f->TR, f->TPART, f->PEND})
    if (p) (void)hipFree(p);
  delete f;
  return 0;
}

int aomarl_field_create(aomarl_ctx *c, int nenv, const aomarl_field_desc *d, aomarl_field **out) {
  if (!c) return fail("field_create: null ctx");
  const EnvView v = env_view(c);
  std::string err;
  if (field_validate_desc(d, field_sys(v), nenv, out, err)) return fail("%s", err.c_str());
  aomarl_field *f = new aomarl_field();
  f->nenv = nenv; f->ndir = d->ndir; f->nlayers = d->nlayers; f->inv_lambda = d->inv_lambda;
  f->W = 2 * v.sys.hw; f->pd = v.sys.pupdiam; f->ref_peak = v.sys.ref_peak;
  f->nblk = (f->pd + FIELD_THREADS / f->W - 1) / (FIELD_THREADS / f->W);
  f->chunk = field_chunk(d->ndir);
  f->off.assign(d->off, d->off + (size_t)2 * d->ndir * d->nlayers);
  f->plan = field_plan(d->ndir);
  const size_t slots = (size_t)nenv * d->ndir, WW = (size_t)f->W * f->W, part = (size_t)nenv * f->chunk;
  struct { float **p; size_t n; } bufs[5] = {{&f->record, slots * 8}, {&f->le, slots * WW}, {&f->TR, part * f->pd * f->W * 2},
                                             {&f->TPART, part * f->nblk * 4}, {&f->PEND, slots * (WW + 4)}};
  for (auto &b : bufs)
    if (hipMalloc((void **)b.p, b.n * sizeof(float)) != hipSuccess || hipMemset(*b.p, 0, b.n * sizeof(float)) != hipSuccess) {
      aomarl_field_destroy(f);
      return fail("field_create: allocating %zu floats failed", b.n);
    }
  HIPCHK(hipDeviceSynchronize());
  *out = f;
  return 0;
}

// what observe and trace share: the refusals, the waits, the deferred shapes; v: the context's view for the launches
static int field_prepare(const char *who, aomarl_field *f, aomarl_ctx *c, aomarl_state *st, int b, int n, int flags, int known,
                         void *stream, EnvView *v) {
  if (!f || !c || !st) return fail("%s: null argument", who);
  int rc = env_refuse_busy(who, c);
  if (rc) return rc;
  *v = env_view(c);
  if (v->nlayers != f->nlayers || v->sys.pupdiam != f->pd || 2 * v->sys.hw != f->W)
    return fail("%s: the field was created on another context (%d layers, pupil %d, window %d)", who, f->nlayers, f->pd, f->W);
  std::string err;
  if (field_validate_call(who, f->nenv, st->nenv, b, n, flags, known, err)) return fail("%s", err.c_str());
  return env_trace_ready(c, st, b, n, flags, stream);
}

int aomarl_field_observe(aomarl_field *f, aomarl_ctx *c, aomarl_state *st, int b, int n, int flags, void *stream) {
  EnvView v;
  int rc = field_prepare("field_observe", f, c, st, b, n, flags, AOMARL_TRACE_ATMOS | AOMARL_TRACE_DMS, stream, &v);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const DevSys &sy = v.sys;
  const DevState ds = dev_state(st);
  DevState fst = ds;                                           // the commit's view: the field's record and sum
  fst.strehl = f->record; fst.le_img = f->le;
  for (const FieldLaunch &L : f->plan) {
    const FieldArgs a = field_args(f->off.data(), f->nlayers, L, v.frac_x, v.frac_y);
    const int kt = field_slots(L.count);
    const size_t sm = sizeof(float) * ((size_t)2 * FIELD_THREADS * kt + FIELD_THREADS + (sy.npsf <= FIELD_TW_LDS ? 2 * (size_t)sy.npsf : 0));
#define FIELD_ROWS(KT)                                                                                                          \
  hipLaunchKernelGGL(k_field_rows<KT>, dim3(f->nblk, n), dim3(FIELD_THREADS), sm, s, sy, ds, a, L.count, f->chunk, f->inv_lambda, b, \
                     flags, f->TR, f->TPART, f->nblk)
#define FIELD_ROWS_ALT(KT)                                                                                                      \
  hipLaunchKernelGGL(k_field_rows_alt<KT>, dim3(f->nblk, n), dim3(FIELD_THREADS), sm, s, sy, ds, a, L.count, f->chunk,        \
                     f->inv_lambda, b, flags, f->TR, f->TPART, f->nblk, ma)
    if (f->mir) {
      const FieldMirArgs ma = field_mir_args(f->mir_base, f->mir_off.data(), L);
      FIELD_DISPATCH(L.count, FIELD_ROWS_ALT);
    } else {
      FIELD_DISPATCH(L.count, FIELD_ROWS);
    }
#undef FIELD_ROWS
#undef FIELD_ROWS_ALT
    LAUNCHCHK();
    hipLaunchKernelGGL(k_field_finish, dim3(L.count, n), dim3(256), 0, s, sy, fst, f->ndir, L.first, f->chunk, b, f->TR, f->TPART,
                       f->nblk, f->PEND);
    LAUNCHCHK();
  }
  return 0;
}

int aomarl_field_trace(aomarl_field *f, aomarl_ctx *c, aomarl_state *st, float *planes, int b, int n, int flags, void *stream) {
  if (!planes) return fail("field_trace: null planes");
  EnvView v;
  int rc = field_prepare("field_trace", f, c, st, b, n, flags,
                         AOMARL_TRACE_ATMOS | AOMARL_TRACE_DMS | AOMARL_TRACE_RESET | AOMARL_TRACE_MASK, stream, &v);
  if (rc) return rc;
  const int np = f->pd * f->pd;
  for (const FieldLaunch &L : f->plan) {
    const FieldArgs a = field_args(f->off.data(), f->nlayers, L, v.frac_x, v.frac_y);
#define FIELD_TRACE(KT)                                                                                                          \
  hipLaunchKernelGGL(k_field_trace<KT>, dim3((np + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, v.sys, dev_state(st), a, \
                     L.count, f->ndir, L.first, planes, b, flags)
#define FIELD_TRACE_ALT(KT)                                                                                                      \
  hipLaunchKernelGGL(k_field_trace_alt<KT>, dim3((np + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, v.sys, dev_state(st), \
                     a, L.count, f->ndir, L.first, planes, b, flags, ma)
    if (f->mir) {
      const FieldMirArgs ma = field_mir_args(f->mir_base, f->mir_off.data(), L);
      FIELD_DISPATCH(L.count, FIELD_TRACE_ALT);
    } else {
      FIELD_DISPATCH(L.count, FIELD_TRACE);
    }
#undef FIELD_TRACE
#undef FIELD_TRACE_ALT
    LAUNCHCHK();
  }
  return 0;
}

int aomarl_field_reset(aomarl_field *f, int b, int n, void *stream) {
  if (!f) return fail("field_reset: null object");
  std::string err;
  if (field_validate_call("field_reset", f->nenv, f->nenv, b, n, 0, 0, err)) return fail("%s", err.c_str());
  // k_strehl_reset on the field's buffers: "environment" e ndir + d
  DevSys sy;
  memset(&sy, 0, sizeof(sy));
  sy.hw = f->W / 2;
  DevState fst;
  memset(&fst, 0, sizeof(fst));
  fst.strehl = f->record; fst.le_img = f->le;
  return launch_strehl_reset(sy, fst, b * f->ndir, n * f->ndir, (hipStream_t)stream);
}

int aomarl_field_get(aomarl_field *f, int do_fit, float **record, float **le, void *stream) {
  if (!f) return fail("field_get: null object");
  if (do_fit) {
    DevSys sy;
    memset(&sy, 0, sizeof(sy));
    sy.hw = f->W / 2; sy.ref_peak = f->ref_peak;
    DevState fst;
    memset(&fst, 0, sizeof(fst));
    fst.strehl = f->record; fst.le_img = f->le;
    // k_strehl_fit_le on the field's buffers: one wave per (environment, direction)
    const int rc = launch_strehl_fit_le(sy, fst, 0, f->nenv * f->ndir, (hipStream_t)stream);
    if (rc) return rc;
  }
  if (record) *record = f->record;
  if (le) *le = f->le;
  return 0;
}

// ---- for aomarl_field_attach_mirrors / _detach_mirrors (aomarl_mcao.hip; aomarl_env_host.h)
void field_dims(const aomarl_field *f, int *nenv, int *ndir, int *pupdiam) { *nenv = f->nenv; *ndir = f->ndir; *pupdiam = f->pd; }

void field_set_mirrors(aomarl_field *f, const aomarl_mcao *owner, const FieldMirArgs &base, const float *off) {
  f->mir_off.assign(off, off + (size_t)2 * f->ndir * base.nmirrors);
  f->mir_base = base;
  f->mir = owner;
}

void field_clear_mirrors(aomarl_field *f) {
  f->mir = nullptr;
  f->mir_off.clear();
}
