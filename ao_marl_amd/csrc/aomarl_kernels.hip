// aomarl_kernels.hip -- CDNA4 (gfx950) kernels of the AO environment hot path: atmosphere, mirrors, raytrace, controller.
// wave = 64 lanes; fp32 MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2_f32) for the GEMM work.
// (the one-pass frame kernel: aomarl_frame.hip; the staged Shack-Hartmann stage: aomarl_wfs.hip; the science target's
// PSF and the Strehl record: aomarl_target.hip)
#include "aomarl_host.h"
#include "aomarl_trace_dev.h"
#include "aomarl_spot_dev.h"          // cvt_h2 .. sub_hi, the split-fp16 operand helpers of aomarl_gemm_nt.h
#include "aomarl_gemm_p.h"
#include <type_traits>

// Arithmetic of the library.  The reference computes in fp32 throughout (Rtc_FFF, shesha/sutra_wrap.py:49; every
// array cast to np.float32, shesha/init/wfs_init.py:76-101), and so does the DEFAULT here: fp32 operands on fp32
// matrix instructions (v_mfma_f32_*_f32), fp32 vector arithmetic.  "precision" = 1 (aomarl_set_precision) is the
// opt-in fast mode: split-fp16 operand pairs (hi + lo, 22-bit mantissa, fp32 accumulation) in the three kernel
// families that have such a form -- the frame kernel's DFTs, the internal GEMMs, the denoiser.
int g_precision = 0;                  // process-wide default of every family (aomarl_set_precision)
// launches per arithmetic family since aomarl_arith_reset (bench.py builds its `dtype` from them)
// (the AR_* enumeration: aomarl_host.h)
unsigned long long g_arith[AR_N] = {0, 0, 0, 0, 0, 0, 0};
static const char *const g_arith_name[AR_N] = {
    "frame_kernel_dft:f32_mfma", "frame_kernel_dft:split_f16_mfma", "gemm:f32_mfma", "gemm:split_f16_mfma",
    "denoiser:f32_mfma", "denoiser:split_f16_mfma", "actor:f32_mfma"};

#include "aomarl_gemm_nt.h"           // the loop's products: k_gemm_nt, k_gemm_nt_h, k_gemm_batched_gen, launch_gemm_nt

// =============================================================================================
// atmosphere: Fried-Clark extrusion on ring-buffered screens
// =============================================================================================
#include "aomarl_move_plan_host.h"    // RoundOps, RoundNext, MoveShift; SG_* and MOVE_SMALL_*: the limits the host plan tests
#include "aomarl_create_plan_host.h"  // DMS_*: the tile of k_dm_shape_sep and the lattice cells it stages

// Z[col][0..ns) = screen[stencil] - zref ; Z[col][ns..ns+n) = amplitude * N(0,1)
// work item j of column col, for a ring origin (ox, oy) and an extrusion counter cnt given by the caller
__device__ __forceinline__ void extrude_gather_item(const DevSys &sys, const DevState &st, int env_begin,
                                                    const RoundOps &ops, float *__restrict__ Z, int ldz,
                                                    float *__restrict__ ZREF, int col, int j, int ox, int oy,
                                                    uint32_t cnt) {
  const int e = env_begin + col / ops.nops, op = col % ops.nops;
  const int li = ops.layer[op], dir = ops.dir[op];
  const DevLayer &L = sys.layers[li];
  const int n = L.dim, ns = L.ns;
  const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
  const bool top_right = (dir == 1 || dir == -2);
  const float zref = base[ring_idx(top_right ? n - 1 : 0, top_right ? 0 : n - 1, ox, oy, n)];
  const uint32_t *ist = ops.tflag[op] ? L.istT : ((dir == 1 || dir == -1) ? L.istx : L.isty);
  const uint32_t seed = st.seeds[e] + (uint32_t)li;
  // items [0, ns): stencil values; items [ns, ns + ceil(n / 4)): 4 normals each (one Philox block)
  if (j < ns) {
    uint32_t xy = ist[j];
    Z[(long long)col * ldz + j] = base[ring_idx(xy & 0xFFFF, xy >> 16, ox, oy, n)] - zref;
  } else if (j < ns + (n + 3) / 4) {
    const int g = j - ns;
    float z4[4];
    philox_normal4(seed, 0u, cnt, 0u, (uint32_t)g, z4);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (4 * g + u < n) Z[(long long)col * ldz + ns + 4 * g + u] = L.amp * z4[u];
  }
  if (j == 0) ZREF[col] = zref;
}

__global__ __launch_bounds__(256) void k_extrude_gather(DevSys sys, DevState st, int env_begin,
                                                        RoundOps ops, float *__restrict__ Z,
                                                        int ldz, float *__restrict__ ZREF) {
  const int col = blockIdx.x;
  const int e = env_begin + col / ops.nops, li = ops.layer[col % ops.nops];
  const int ox = st.origin[(e * sys.nlayers + li) * 2], oy = st.origin[(e * sys.nlayers + li) * 2 + 1];
  extrude_gather_item(sys, st, env_begin, ops, Z, ldz, ZREF, col, blockIdx.y * blockDim.x + threadIdx.x, ox, oy,
                      st.ext_count[e * sys.nlayers + li]);
}

// new line -> ring (+ mirror columns) for a ring origin (ox, oy); returns the advanced origin
__device__ __forceinline__ void extrude_scatter_col(const DevSys &sys, const DevState &st, int env_begin,
                                                    const RoundOps &ops, const float *__restrict__ NEWL, int ldn,
                                                    const float *__restrict__ ZREF, const float *__restrict__ P,
                                                    int nsplit, int ncol, int pn, float pscale, int col, int ox,
                                                    int oy, int &nox, int &noy, float *__restrict__ snew = nullptr) {
  // nsplit > 0: the new lines are still split-K partial tiles P[z][ncol][pn] of the extrusion GEMM
  // (times 1 / pscale when the split-f16 kernel produced them from scaled operands)
  const int e = env_begin + col / ops.nops, op = col % ops.nops;
  const int li = ops.layer[op], dir = ops.dir[op];
  const DevLayer &L = sys.layers[li];
  const int n = L.dim;
  float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
  const float zref = ZREF[col];
  const int stride = n + RING_PAD;
  for (int r = threadIdx.x; r < n; r += blockDim.x) {
    float v = zref;
    if (nsplit > 0) {
      const float acc = slab_sum<8>(nsplit, [&](int z) { return P[((long long)z * ncol + col) * pn + r]; });   // (tools/reset_trace.sh)
      v += acc * pscale;
    } else {
      v += NEWL[(long long)col * ldn + r];
    }
    int px, py;
    if (dir == 1) {
      px = ox;
      py = r + oy; py -= (py >= n) ? n : 0;
    } else if (dir == -1) {
      px = ox - 1; px += (px < 0) ? n : 0;
      py = n - 1 - r + oy; py -= (py >= n) ? n : 0;
    } else if (dir == 2) {
      py = oy;
      px = r + ox; px -= (px >= n) ? n : 0;
    } else {
      py = oy - 1; py += (py < 0) ? n : 0;
      px = n - 1 - r + ox; px -= (px >= n) ? n : 0;
    }
    base[py * stride + px] = v;
    if (px < RING_PAD) base[py * stride + n + px] = v;     // mirror columns
    if (snew) snew[r] = v;                                 // (k_extrude_sg: the next stencil's points on this line)
  }
  nox = ox; noy = oy;
  if (dir == 1) nox = (ox + 1 >= n) ? 0 : ox + 1;
  else if (dir == -1) nox = (ox - 1 < 0) ? n - 1 : ox - 1;
  else if (dir == 2) noy = (oy + 1 >= n) ? 0 : oy + 1;
  else noy = (oy - 1 < 0) ? n - 1 : oy - 1;
}

// new line -> ring, then the ring origin / extrusion counter of this (environment, layer) advance:
// one block per column, so nobody else reads that origin
__global__ __launch_bounds__(256) void k_extrude_scatter(DevSys sys, DevState st, int env_begin,
                                                         RoundOps ops,
                                                         const float *__restrict__ NEWL, int ldn,
                                                         const float *__restrict__ ZREF,
                                                         const float *__restrict__ P, int nsplit,
                                                         int ncol, int pn, float pscale) {
  const int col = blockIdx.x;
  const int e = env_begin + col / ops.nops, li = ops.layer[col % ops.nops];
  int *o = st.origin + (e * sys.nlayers + li) * 2;
  const int ox = o[0], oy = o[1];
  int nox, noy;
  extrude_scatter_col(sys, st, env_begin, ops, NEWL, ldn, ZREF, P, nsplit, ncol, pn, pscale, col, ox, oy, nox, noy);
  __syncthreads();
  if (threadIdx.x == 0) {
    o[0] = nox; o[1] = noy;
    if (st.origin_snap) { st.origin_snap[(e * sys.nlayers + li) * 2] = nox; st.origin_snap[(e * sys.nlayers + li) * 2 + 1] = noy; }
    st.ext_count[e * sys.nlayers + li] += 1u;
  }
}

// scatter of round r and gather of round r + 1 in one launch: the dependency is column-local -- a
// column's next stencil reads only that column's screen, including the line just written -- so one
// block does both, with the advanced origin and counter carried in registers (never re-read: a
// uniform re-load could come from the scalar cache, which the block's own stores do not update).
// The next round may hold fewer layers (a frame's rounds thin out as the slower layers finish) and other
// directions: `nx` says where this column's layer sits in it; its Z / ZREF are a second pair of buffers
// (ZN / ZREFN: the next round numbers its columns anew, another block may still need this round's ZREF entry).
// (SG_MAX_N: the longest line kept in LDS; SG_THREADS threads per column, SG_U stencil items per thread: checked on the host)
__global__ __launch_bounds__(SG_THREADS) void k_extrude_sg(DevSys sys, DevState st, int env_begin, RoundOps ops,
                                                    const float *__restrict__ NEWL, int ldn,
                                                    const float *__restrict__ ZREF, const float *__restrict__ P,
                                                    int nsplit, int ncol, int pn, float pscale,
                                                    float *__restrict__ Z, int ldz, float *__restrict__ ZREFN,
                                                    RoundNext nx) {
  __shared__ float snew[SG_MAX_N];               // the line this block writes, for the next stencil's points on it
  const int col = blockIdx.x;
  const int el = col / ops.nops, oi = col % ops.nops;
  const int e = env_begin + el, li = ops.layer[oi];
  int *o = st.origin + (e * sys.nlayers + li) * 2;
  const int ox = o[0], oy = o[1];
  const uint32_t cnt = st.ext_count[e * sys.nlayers + li];
  const DevLayer &L = sys.layers[li];
  const int n = L.dim, ns = L.ns;
  const int ni = nx.idx[oi];                     // this column's layer in the next round (-1: it has no operation there)
  const int col2 = el * nx.nops + (ni < 0 ? 0 : ni);
  const int dir = nx.dir[ni < 0 ? 0 : ni];
  // the origin as this round's scatter leaves it (the same arithmetic as extrude_scatter_col's)
  const int cdir = ops.dir[oi];
  int eox = ox, eoy = oy;
  if (cdir == 1) eox = (ox + 1 >= n) ? 0 : ox + 1;
  else if (cdir == -1) eox = (ox - 1 < 0) ? n - 1 : ox - 1;
  else if (cdir == 2) eoy = (oy + 1 >= n) ? 0 : oy + 1;
  else eoy = (oy - 1 < 0) ? n - 1 : oy - 1;
  // Is the logical point (x, y) of the ADVANCED screen on the line this block is about to write, and which of its
  // elements is it?  (dir +1: the new column is x = n - 1, element y; -1: x = 0, element n - 1 - y; +2: the row y = n - 1,
  // element x; -2: y = 0, element n - 1 - x -- the placement rules of extrude_scatter_col)
  auto on_new = [&](int x, int y, int &r) {
    if (cdir == 1) { r = y; return x == n - 1; }
    if (cdir == -1) { r = n - 1 - y; return x == 0; }
    if (cdir == 2) { r = x; return y == n - 1; }
    r = n - 1 - x; return y == 0;
  };
  // What the next round's gather needs and the scatter does not touch goes FIRST, so that it runs while the scatter's
  // loads are in flight instead of behind the barrier: the stencil's index list (the gather was a dependent pair of
  // loads per item), the noise half of Z (Philox + two Box-Muller pairs per item: nothing but arithmetic) and -- round
  // 6 -- the stencil's VALUES off the new line: half of the stencil (its second full line and the far points) is older
  // data that this block does not write, and the other half IS the line it writes, which it keeps in LDS: no value is
  // read back from the ring behind the barrier, one dependent round trip to memory less per launch.  Z / ZREFN are the
  // next round's buffers: the product that last read them is a whole round back.
  constexpr int U = SG_U;                        // ns <= U * blockDim.x (checked on the host: AOMARL_SG_MAX_NS)
  const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
  float v[U] = {};
  int rr[U] = {};
  bool nw[U] = {};
  float zref = 0.f;
  int zr = 0;
  bool znew = false;
  if (ni >= 0) {
    const uint32_t *ist = nx.tflag[ni] ? L.istT : ((dir == 1 || dir == -1) ? L.istx : L.isty);
    uint32_t xy[U];
#pragma unroll
    for (int u = 0; u < U; u++) xy[u] = ist[min((int)threadIdx.x + u * (int)blockDim.x, ns - 1)];
    const bool top_right = (dir == 1 || dir == -2);
    const int zx = top_right ? n - 1 : 0, zy = top_right ? 0 : n - 1;
    znew = on_new(zx, zy, zr);
    if (!znew) zref = base[ring_idx(zx, zy, eox, eoy, n)];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int x = xy[u] & 0xFFFF, y = xy[u] >> 16;
      nw[u] = on_new(x, y, rr[u]);
      if (!nw[u]) v[u] = base[ring_idx(x, y, eox, eoy, n)];
    }
    const uint32_t seed = st.seeds[e] + (uint32_t)li;
    for (int g = threadIdx.x; g < (n + 3) / 4; g += blockDim.x) {
      float z4[4];
      philox_normal4(seed, 0u, cnt + 1u, 0u, (uint32_t)g, z4);
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (4 * g + u < n) Z[(long long)col2 * ldz + ns + 4 * g + u] = L.amp * z4[u];
    }
  }
  int nox, noy;
  extrude_scatter_col(sys, st, env_begin, ops, NEWL, ldn, ZREF, P, nsplit, ncol, pn, pscale, col, ox, oy, nox, noy, snew);
  __syncthreads();                               // the new line is in the ring and in LDS; ZREF[col] was read by everyone
  if (threadIdx.x == 0) {
    o[0] = nox; o[1] = noy;
    if (st.origin_snap) { st.origin_snap[(e * sys.nlayers + li) * 2] = nox; st.origin_snap[(e * sys.nlayers + li) * 2 + 1] = noy; }
    st.ext_count[e * sys.nlayers + li] = cnt + 1u;
  }
  if (ni < 0) return;
  if (znew) zref = snew[zr];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = (int)threadIdx.x + u * (int)blockDim.x;
    if (nw[u]) v[u] = snew[rr[u]];
    if (j < ns) Z[(long long)col2 * ldz + j] = v[u] - zref;
  }
  if (threadIdx.x == 0) ZREFN[col2] = zref;
}

// Small screens (dim <= 256, ns + dim <= MOVE_SMALL_K): ALL the extrusions of one frame's move in ONE launch.
// One block per (environment, layer): per extrusion it gathers Z = [stencil - zref | amp N(0,1)] into LDS,
// forms the new line zref + [A|B] Z from the transposed matrix (thread = (row, K slice), coalesced over
// rows, the K slices summed in a fixed order through LDS), writes it into the ring and goes on with the
// origin and counter it carries in registers: |kx| x-extrusions, then |ky| y-extrusions, as move_round
// orders them.  The matrix (a few hundred KB) is re-read from L2 by every block, which is what limits
// this to small screens: there the step is bound by the host's launches (configs[1]: 6 - 12 launches of
// the generic rounds become 1), not by the arithmetic.  fp32 vector FMAs in both precision modes.
__global__ __launch_bounds__(MOVE_SMALL_T) void k_move_small(DevSys sys, DevState st, int env_begin, MoveShift plan) {
  __shared__ float Zs[MOVE_SMALL_K];
  __shared__ __attribute__((aligned(16))) float Ps[4 * MOVE_SMALL_T];     // parts x ldt partial sums
  const int e = env_begin + blockIdx.x, li = blockIdx.y, tid = threadIdx.x;
  const int kx = plan.kx[li], ky = plan.ky[li];
  const int nx = abs(kx), nit = nx + abs(ky);
  if (nit == 0) return;
  const DevLayer &L = sys.layers[li];
  const int n = L.dim, ns = L.ns, K = n + ns, stride = n + RING_PAD, ldt = L.ldt;
  // thread = (group of 4 rows, K slice): one 16-byte load of the transposed matrix per k, ldt / 4 row groups,
  // 4 * MOVE_SMALL_T / ldt slices (8 .. 32): many independent loads in flight per thread instead of one per row
  const int rgs = ldt >> 2, parts = MOVE_SMALL_T / rgs, part = tid / rgs, rg = tid - part * rgs;
  float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
  int *o = st.origin + (e * sys.nlayers + li) * 2;
  int ox = o[0], oy = o[1];
  uint32_t cnt = st.ext_count[e * sys.nlayers + li];
  const uint32_t seed = st.seeds[e] + (uint32_t)li;
  const float amp = L.amp;
  const float *__restrict__ ABt = L.ABt;
  for (int it = 0; it < nit; it++) {
    const int dir = it < nx ? (kx > 0 ? 1 : -1) : (ky > 0 ? 2 : -2);
    const bool top_right = (dir == 1 || dir == -2);
    // the ring is rewritten by this block between iterations: a plain vector load, never the scalar cache
    const float zref = __hip_atomic_load(base + ring_idx(top_right ? n - 1 : 0, top_right ? 0 : n - 1, ox, oy, n),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint32_t *ist = (dir == 1 || dir == -1) ? L.istx : L.isty;
    for (int j = tid; j < ns; j += MOVE_SMALL_T) {
      const uint32_t xy = ist[j];
      Zs[j] = __hip_atomic_load(base + ring_idx(xy & 0xFFFF, xy >> 16, ox, oy, n), __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_WORKGROUP) - zref;
    }
    for (int g = tid; g < (n + 3) / 4; g += MOVE_SMALL_T) {
      float z4[4];
      philox_normal4(seed, 0u, cnt, 0u, (uint32_t)g, z4);
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (4 * g + u < n) Zs[ns + 4 * g + u] = amp * z4[u];
    }
    __syncthreads();
    if (part < parts) {
      float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
      const float4 *p = reinterpret_cast<const float4 *>(ABt) + rg;
      auto acc = [](float4 &a, const float4 m, float z) {
        a.x = fmaf(m.x, z, a.x); a.y = fmaf(m.y, z, a.y); a.z = fmaf(m.z, z, a.z); a.w = fmaf(m.w, z, a.w);
      };
      int j = part;
      for (; j + 3 * parts < K; j += 4 * parts) {
        const float4 m0 = p[(long long)j * rgs], m1 = p[(long long)(j + parts) * rgs];
        const float4 m2 = p[(long long)(j + 2 * parts) * rgs], m3 = p[(long long)(j + 3 * parts) * rgs];
        acc(a0, m0, Zs[j]); acc(a1, m1, Zs[j + parts]); acc(a2, m2, Zs[j + 2 * parts]); acc(a3, m3, Zs[j + 3 * parts]);
      }
      for (; j < K; j += parts) acc(a0, p[(long long)j * rgs], Zs[j]);
      float4 t;
      t.x = (a0.x + a1.x) + (a2.x + a3.x); t.y = (a0.y + a1.y) + (a2.y + a3.y);
      t.z = (a0.z + a1.z) + (a2.z + a3.z); t.w = (a0.w + a1.w) + (a2.w + a3.w);
      reinterpret_cast<float4 *>(Ps)[part * rgs + rg] = t;
    }
    __syncthreads();
    if (tid < n) {
      float v = 0.f;
      for (int q = 0; q < parts; q++) v += Ps[q * ldt + tid];
      v += zref;
      const int r = tid;
      int px, py;
      if (dir == 1) {
        px = ox;
        py = r + oy; py -= (py >= n) ? n : 0;
      } else if (dir == -1) {
        px = ox - 1; px += (px < 0) ? n : 0;
        py = n - 1 - r + oy; py -= (py >= n) ? n : 0;
      } else if (dir == 2) {
        py = oy;
        px = r + ox; px -= (px >= n) ? n : 0;
      } else {
        py = oy - 1; py += (py < 0) ? n : 0;
        px = n - 1 - r + ox; px -= (px >= n) ? n : 0;
      }
      base[py * stride + px] = v;
      if (px < RING_PAD) base[py * stride + n + px] = v;     // mirror columns
    }
    if (dir == 1) ox = (ox + 1 >= n) ? 0 : ox + 1;
    else if (dir == -1) ox = (ox - 1 < 0) ? n - 1 : ox - 1;
    else if (dir == 2) oy = (oy + 1 >= n) ? 0 : oy + 1;
    else oy = (oy - 1 < 0) ? n - 1 : oy - 1;
    cnt += 1u;
    __syncthreads();                             // the new line is in the ring (block-visible); Zs / Ps are free again
  }
  if (tid == 0) {
    o[0] = ox; o[1] = oy;
    if (st.origin_snap) { st.origin_snap[(e * sys.nlayers + li) * 2] = ox; st.origin_snap[(e * sys.nlayers + li) * 2 + 1] = oy; }
    st.ext_count[e * sys.nlayers + li] = cnt;
  }
}

// in-place transposition of the n x n ring of (environment, layer li): 32 x 32 tiles, block = the tile
// pair (i, j) / (j, i), i <= j; the ring origin is exchanged with it.  The mirror columns are rebuilt by
// k_refresh_mirror afterwards.
__global__ __launch_bounds__(256) void k_transpose_ring(DevSys sys, DevState st, int env_begin, int li, int T) {
  __shared__ float A[32][33], B[32][33];
  const DevLayer &L = sys.layers[li];
  const int n = L.dim, stride = n + RING_PAD;
  const int e = env_begin + blockIdx.y;
  float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
  // pair index -> (i, j), i <= j (row-major over the upper triangle)
  int k = blockIdx.x, i = 0;
  while (k >= T - i) { k -= T - i; i++; }
  const int j = i + k;
  const int tx = threadIdx.x & 31, ty0 = threadIdx.x >> 5;
  for (int ty = ty0; ty < 32; ty += 8) {
    const int ya = 32 * i + ty, xa = 32 * j + tx;          // tile (i, j): rows of tile row i, columns of tile column j
    const int yb = 32 * j + ty, xb = 32 * i + tx;
    A[ty][tx] = (ya < n && xa < n) ? base[ya * stride + xa] : 0.f;
    B[ty][tx] = (yb < n && xb < n) ? base[yb * stride + xb] : 0.f;
  }
  __syncthreads();
  for (int ty = ty0; ty < 32; ty += 8) {
    const int ya = 32 * i + ty, xa = 32 * j + tx;
    const int yb = 32 * j + ty, xb = 32 * i + tx;
    if (ya < n && xa < n) base[ya * stride + xa] = B[tx][ty];
    if (i != j && yb < n && xb < n) base[yb * stride + xb] = A[tx][ty];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int *o = st.origin + (e * sys.nlayers + li) * 2;
    const int ox = o[0], oy = o[1];
    o[0] = oy; o[1] = ox;
  }
}

__global__ void k_refresh_mirror(DevSys sys, DevState st, int env_begin, int li) {
  const DevLayer &L = sys.layers[li];
  const int n = L.dim, stride = n + RING_PAD;
  const int e = env_begin + blockIdx.y;
  float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n * RING_PAD) return;
  const int y = p / RING_PAD, x = p - y * RING_PAD;
  base[y * stride + n + x] = base[y * stride + x];
}

__global__ void k_fill_f32(float *p, long long n, float v) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

__global__ void k_reset_env(DevSys sys, DevState st, int env_begin, int env_count,
                            const uint32_t *__restrict__ seeds_dev, int ld_actu, int origin_in_y) {
  // small per-env state: origin, counters, integrator vectors
  const int e = env_begin + blockIdx.x;
  if (threadIdx.x == 0) {
    st.seeds[e] = seeds_dev[blockIdx.x];
    st.frame[e] = 0u;
  }
  for (int i = threadIdx.x; i < sys.nlayers; i += blockDim.x) {
    // Where the ring starts is free (the logical screen does not depend on it).  Start it so that the first pupil
    // pixel of a row sits on a 128-byte line once the reset is through: the frame kernel's 32-pixel pieces of a layer
    // that does not move along x (ground layers under a wind along y: this ring origin never changes) then ARE whole
    // lines, for the whole episode.  The reset's 2 dim extrusions bring the origin back to where it started, and its
    // final transposition exchanges x and y (origin_in_y: start the offset in y).
    const int a = sys.fused_ok ? (32 - (sys.layers[i].tox & 31)) & 31 : 0;
    st.origin[(e * sys.nlayers + i) * 2] = origin_in_y ? 0 : a;
    st.origin[(e * sys.nlayers + i) * 2 + 1] = origin_in_y ? a : 0;
    st.ext_count[e * sys.nlayers + i] = 0u;
  }
  for (int i = threadIdx.x; i < ld_actu; i += blockDim.x) {
    long long o = (long long)e * ld_actu + i;
    st.com[o] = 0.f; st.com1[o] = 0.f; st.com2[o] = 0.f; st.err[o] = 0.f; st.voltage[o] = 0.f;
  }
}

// upload logical screens src [env_count][n*n] (origin reset to 0, mirror columns filled)
__global__ void k_set_screen(DevSys sys, DevState st, int env_begin, int li, const float *src) {
  const DevLayer &L = sys.layers[li];
  const int n = L.dim, stride = n + RING_PAD;
  const int e = env_begin + blockIdx.y;
  float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n * stride; p += gridDim.x * blockDim.x) {
    int y = p / stride, x = p - y * stride;
    base[p] = src[(long long)blockIdx.y * n * n + y * n + (x >= n ? x - n : x)];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st.origin[(e * sys.nlayers + li) * 2] = 0;
    st.origin[(e * sys.nlayers + li) * 2 + 1] = 0;
  }
}

__global__ void k_get_screen(DevSys sys, DevState st, int env_begin, int li, float *dst) {
  const DevLayer &L = sys.layers[li];
  const int n = L.dim;
  const int e = env_begin + blockIdx.y;
  const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
  const int ox = st.origin[(e * sys.nlayers + li) * 2], oy = st.origin[(e * sys.nlayers + li) * 2 + 1];
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n * n; p += gridDim.x * blockDim.x) {
    int y = p / n, x = p - y * n;
    dst[(long long)blockIdx.y * n * n + p] = base[ring_idx(x, y, ox, oy, n)];
  }
}

// =============================================================================================
// deformable mirrors (dm_value, what a consumer reads of a mirror: aomarl_trace_dev.h)
// =============================================================================================
// tip-tilt mirror k of environment env_begin + row: its two coefficients, and (p == 2) the stack-array
// DM's value at the centre of the pupil grid
__device__ __forceinline__ void dm_shape_tt_body(const DevSys &sys, const DevState &st, int env_begin, int row, int k,
                                                 const float *__restrict__ volts, int ldv, int p) {
  const DevDm &D = sys.dms[k];
  const float *com = volts + (long long)row * ldv + D.com_off;
  float *shape = st.dm_shape + (long long)(env_begin + row) * sys.shape_stride + D.shape_off;
  if (p < 2) shape[p] = com[p];
  if (p == 2 && sys.fused_ok) {
    // stack-array DM value at the centre of the pupil grid (pivot of the one-pass frame kernel's
    // variance sums when the stack-array shape is evaluated from the commands on the fly)
    const DevDm &Z = sys.dms[0];
    const float *zc = volts + (long long)row * ldv + Z.com_off;
    const int half = sys.pupdiam / 2, zp = (half + Z.toy) * Z.dim + half + Z.tox;
    const int ss2 = Z.ss * Z.ss, s0 = Z.influstart[zp], cn = Z.ninflu[zp];
    float acc = 0.f;
    for (int t = 0; t < cn; t++) {
      const int pos = Z.influpos[s0 + t];
      acc += Z.influ[pos] * zc[pos / ss2];
    }
    shape[2] = acc;
  }
}

// generic per-pixel gather over the reference's influpos / ninflu / influstart tables
__global__ __launch_bounds__(256) void k_dm_shape(DevSys sys, DevState st, int env_begin, int k,
                                                  const float *__restrict__ volts, int ldv) {
  const DevDm &D = sys.dms[k];
  const int e = env_begin + blockIdx.y;
  const float *com = volts + (long long)blockIdx.y * ldv + D.com_off;
  float *shape = st.dm_shape + (long long)e * sys.shape_stride + D.shape_off;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (D.type == AOMARL_DM_TT) {
    dm_shape_tt_body(sys, st, env_begin, blockIdx.y, k, volts, ldv, p);
    return;
  }
  if (p >= D.dim * D.dim) return;
  const int ss2 = D.ss * D.ss;
  const int s0 = D.influstart[p], c = D.ninflu[p];
  float acc = 0.f;
  for (int t = 0; t < c; t++) {
    int pos = D.influpos[s0 + t];
    acc += D.influ[pos] * com[pos / ss2];
  }
  shape[p] = acc;
}

// separable lattice fast path: tile of 64 x 32 pixels per block; the <= 9 x 8 lattice cells that
// can reach the tile are staged in LDS; shape = sum_gy u(y - Yg) sum_gx u(x - Xg) C[gy][gx]
// (DMS_TX / TY / GX / GY: aomarl_create_plan_host.h, the limits the creation plan tests)
__global__ __launch_bounds__(256) void k_dm_shape_sep(DevSys sys, DevState st, int env_begin, int k,
                                                      const float *__restrict__ volts, int ldv) {
  __shared__ float sC[DMS_GY][DMS_GX + 1];
  __shared__ float sU[128];
  const DevDm &D = sys.dms[k];
  const int e = env_begin + blockIdx.z;
  const float *com = volts + (long long)blockIdx.z * ldv + D.com_off;
  float *shape = st.dm_shape + (long long)e * sys.shape_stride + D.shape_off;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * DMS_TX, y0 = blockIdx.y * DMS_TY;
  const int ss = D.ss, pitch = D.pitch;
  // first lattice column / row that can touch the tile: X_g + ss - 1 >= x0
  auto first = [&](int p0, int pmin) {
    int num = p0 - pmin - (ss - 1);
    int g = num >= 0 ? (num + pitch - 1) / pitch : -((-num) / pitch);
    return g;
  };
  const int gxb = first(x0, D.i1min), gyb = first(y0, D.j1min);
  if (tid < ss) sU[tid] = D.prof[tid];
  if (tid < DMS_GY * DMS_GX) {
    const int r = tid / DMS_GX, cc = tid - r * DMS_GX;
    const int gx = gxb + cc, gy = gyb + r;
    float v = 0.f;
    if (gx >= 0 && gx < D.gw && gy >= 0 && gy < D.gh) {
      int a = D.grid[gy * D.gw + gx];
      if (a >= 0) v = com[a];
    }
    sC[r][cc] = v;
  }
  __syncthreads();
  const int x = x0 + (tid & 63);
  float wx[DMS_GX];
#pragma unroll
  for (int cc = 0; cc < DMS_GX; cc++) {
    int a = x - (D.i1min + pitch * (gxb + cc));
    wx[cc] = (a >= 0 && a < ss) ? sU[a] : 0.f;
  }
  float rs[DMS_GY];
#pragma unroll
  for (int r = 0; r < DMS_GY; r++) {
    float acc = 0.f;
#pragma unroll
    for (int cc = 0; cc < DMS_GX; cc++) acc += wx[cc] * sC[r][cc];
    rs[r] = acc;
  }
  if (x >= D.dim) return;
#pragma unroll
  for (int j = 0; j < DMS_TY / 4; j++) {
    const int y = y0 + (tid >> 6) + 4 * j;
    if (y >= D.dim) continue;
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < DMS_GY; r++) {
      int a = y - (D.j1min + pitch * (gyb + r));
      float wy = (a >= 0 && a < ss) ? sU[a] : 0.f;
      acc += wy * rs[r];
    }
    shape[y * D.dim + x] = acc;
  }
}

// materialise any DM's shape into dst [env_count][dim*dim] (getter for tests / host API)
__global__ void k_get_dm_shape(DevSys sys, DevState st, int env_begin, int k, float *dst) {
  const DevDm &D = sys.dms[k];
  const int e = env_begin + blockIdx.y;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < D.dim * D.dim; p += gridDim.x * blockDim.x) {
    int y = p / D.dim, x = p - y * D.dim;
    dst[(long long)blockIdx.y * D.dim * D.dim + p] = dm_value(sys, st, e, k, x, y);
  }
}

// =============================================================================================
// raytrace into a phase buffer (generic, bilinear) -- unfused API path (bilinear_ring, trace_dms: aomarl_trace_dev.h)
// =============================================================================================
template <bool TARGET>
__global__ __launch_bounds__(256) void k_raytrace(DevSys sys, DevState st, int env_begin,
                                                  int flags) {
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
      v += bilinear_ring(base, L.dim, ox, oy, (float)x + (TARGET ? L.txo : L.wxo),
                         (float)y + (TARGET ? L.tyo : L.wyo));
    }
  }
  if (flags & AOMARL_TRACE_DMS) {
    v = trace_dms<TARGET>(sys, st, e, x, y, v);
  }
  if (flags & AOMARL_TRACE_MASK) v *= (TARGET ? sys.spupil : sys.mpupil)[p];
  out[p] = v;
}

// =============================================================================================
// controller glue
// =============================================================================================
// com += gain * err     (err = -cmat.s was produced by the GEMM with alpha = -1)
__global__ void k_integrate(float *__restrict__ com, const float *__restrict__ err, int nactu,
                            int ld, float gain, int env_begin, const float *__restrict__ env_gain) {
  const int e = env_begin + blockIdx.y;
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a < nactu) com[(long long)e * ld + a] += (env_gain ? env_gain[e] : gain) * err[(long long)e * ld + a];
}

// voltage = a com + b com1 + c com2 ; com2 <- com1 ; com1 <- com
__global__ void k_delay(DevState st, int nactu, int ld, float a, float b, float c, int env_begin,
                        int comp_voltage) {
  const int e = env_begin + blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nactu) return;
  const long long o = (long long)e * ld + i;
  const float c0 = st.com[o];
  if (comp_voltage) {
    const float c1 = st.com1[o], c2 = st.com2[o];
    st.voltage[o] = a * c0 + b * c1 + c * c2;
    st.com2[o] = c1;
    st.com1[o] = c0;
  } else {
    st.voltage[o] = c0;
  }
}

// k_delay whose newest command is still the split-K partial tiles P[z][n][nactu] of the m2v product:
// com = alpha * sum_z P[z] (k_gemm_reduce's expression, same order), then the delay line
__global__ void k_delay_sum(DevState st, int nactu, int ld, float a, float b, float c, int env_begin,
                            int comp_voltage, const float *__restrict__ P, int nsplit, float alpha, int nrows) {
  const int e = env_begin + blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nactu) return;
  const long long o = (long long)e * ld + i;
  const float s = slab_sum<4>(nsplit, [&](int z) { return P[((long long)z * nrows + blockIdx.y) * nactu + i]; });
  const float c0 = alpha * s;
  st.com[o] = c0;
  if (comp_voltage) {
    const float c1 = st.com1[o], c2 = st.com2[o];
    st.voltage[o] = a * c0 + b * c1 + c * c2;
    st.com2[o] = c1;
    st.com1[o] = c0;
  } else {
    st.voltage[o] = c0;
  }
}

// Frame pipeline, loop delay of exactly one frame: the voltages of the NEXT frame are the new commands
// (k_delay's expression with weights (0, 1, 0), evaluated one shift earlier), the delay line shifts, and the
// tip-tilt slot of that frame's dm_shape is filled by the same launch (rows >= n: dm_shape_tt_body with the
// voltages it needs recomputed by the rows' own expression), so that the frame kernel waits for ONE kernel
// behind the m2v product.  P: split-K partial tiles of that product (nsplit > 0) or null (st.com holds it).
__global__ void k_delay_ahead(DevSys sys, DevState st, int nactu, int ld, int n, const float *__restrict__ P,
                              int nsplit, float alpha, int ktt) {
  auto newest = [&](int row, int a) -> float {
    if (nsplit > 0) {
      return alpha * slab_sum<4>(nsplit, [&](int z) { return P[((long long)z * n + row) * nactu + a]; });
    }
    return st.com[(long long)row * ld + a];
  };
  if ((int)blockIdx.y < n) {
    const int e = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nactu) return;
    const long long o = (long long)e * ld + i;
    const float c0 = newest(e, i);
    if (nsplit > 0) st.com[o] = c0;
    const float c1 = st.com1[o];
    st.voltage[o] = c0;
    st.com2[o] = c1;
    st.com1[o] = c0;
  } else if (blockIdx.x == 0 && ktt >= 0) {
    const int row = blockIdx.y - n, p = threadIdx.x;
    const DevDm &D = sys.dms[ktt];
    float *shape = st.dm_shape + (long long)row * sys.shape_stride + D.shape_off;
    if (p < 2) shape[p] = newest(row, D.com_off + p);
    if (p == 2 && sys.fused_ok) {
      const DevDm &Z = sys.dms[0];
      const int half = sys.pupdiam / 2, zp = (half + Z.toy) * Z.dim + half + Z.tox;
      const int ss2 = Z.ss * Z.ss, s0 = Z.influstart[zp], cn = Z.ninflu[zp];
      float acc = 0.f;
      for (int t = 0; t < cn; t++) {
        const int pos = Z.influpos[s0 + t];
        acc += Z.influ[pos] * newest(row, Z.com_off + pos / ss2);
      }
      shape[2] = acc;
    }
  }
}

__global__ void k_copy_rows(float *__restrict__ dst, int ldd, const float *__restrict__ src,
                            int lds, int ncols) {
  const int r = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncols) dst[(long long)r * ldd + i] = src[(long long)r * lds + i];
}

// modes[e][action_modes[j]] += action[e][j] * freedom[action_modes[j]]
__global__ void k_modal_add(float *__restrict__ modes, int ldm, const float *__restrict__ action,
                            int nact, const int32_t *__restrict__ amodes,
                            const float *__restrict__ freedom) {
  const int r = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < nact) {
    int m = amodes[j];
    modes[(long long)r * ldm + m] += action[(long long)r * nact + j] * freedom[m];
  }
}

// What follows the delay line in one launch: blocks [0, n) commit the pending PSF window (k_strehl_commit),
// blocks [n, 2n) refresh the tip-tilt mirror's coefficients and the frame kernel's pivot from the
// new voltages (k_dm_shape's tip-tilt branch).  The two halves touch different data.
__global__ __launch_bounds__(256) void k_post_delay(DevSys sys, DevState st, int env_begin, int n,
                                                    const float *__restrict__ PEND, int do_strehl, int ktt,
                                                    const float *__restrict__ volts, int ldv) {
  if ((int)blockIdx.x < n) {
    if (do_strehl) strehl_commit_body(sys, st, env_begin, blockIdx.x, PEND);
  } else {
    dm_shape_tt_body(sys, st, env_begin, blockIdx.x - n, ktt, volts, ldv, threadIdx.x);
  }
}
