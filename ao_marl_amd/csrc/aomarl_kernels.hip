// aomarl_kernels.hip -- CDNA4 (gfx950) kernels of the AO environment hot path.
// wave = 64 lanes; fp32 MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2_f32) for the DFT and GEMM work.
#include "aomarl_host.h"
#include "aomarl_trace_dev.h"
#include "aomarl_spot_dev.h"          // cvt_h2 .. add4_ring, the spot of one sub-aperture: shared with aomarl_frame.hip
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
// Shack-Hartmann spot image + centre of gravity.
// One wavefront per (environment, sub-aperture); specialised for the production sampling
// pdiam = 16 phase pixels, Nfft = 64, nrebin = 2, npix = 16 (SURVEY Appendix A / golden fixtures).
//
// The 16x16 complex pupil tile is staged in LDS; the zero-padded 64x64 FFT is never formed:
// only the 32x32 central frequencies feed the 16x16 binned image, and the input has 16 non-zero
// rows/columns, so the transform is the pruned DFT  X = E^T . a . E  with E[16][32] =
// exp(-2 pi i x k / 64), k in [-16, 16): two small complex GEMMs (96 v_mfma_f32_16x16x4_f32).
// |X|^2, the 2x2 binning (binmap), the flux normalisation, optional noise and the COG are done on
// the accumulator registers (spot_compute and what it is made of: aomarl_spot_dev.h).
// =============================================================================================

// phase (sum of all sources) and pupil mask of the 4 pixels this lane owns in sub-aperture i
template <bool FROM_BUF>
__device__ __forceinline__ void spot_load(const DevSys &sys, const DevState &st, int e, int i,
                                          int lane, int no_atmos, int no_dms, float ph[4],
                                          float mk[4]) {
  const int xy0 = sys.sub_xy[i];
  const int gx0 = xy0 & 0xFFFF, gy0 = xy0 >> 16;
  const int ty = lane >> 2, tx0 = (lane & 3) * 4;
  const int gy = gy0 + ty;
#pragma unroll
  for (int j = 0; j < 4; j++) { ph[j] = 0.f; mk[j] = 0.f; }
  if (FROM_BUF) {
    add4(ph, st.wfs_phase + (long long)e * sys.n * sys.n + gy * sys.n + gx0 + tx0);
  } else {
    if (!no_atmos) {
      for (int l = 0; l < sys.nlayers; l++) {
        const DevLayer &L = sys.layers[l];
        const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
        const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
        int py = gy + L.woy + oy; py -= (py >= L.dim) ? L.dim : 0;
        int px = gx0 + tx0 + L.wox + ox; px -= (px >= L.dim) ? L.dim : 0;
        add4_ring(ph, base + py * (L.dim + RING_PAD), px, L.dim);
      }
    }
    if (!no_dms) {
      for (int k = 0; k < sys.ndm; k++) {
        const DevDm &D = sys.dms[k];
        const float *slot = st.dm_shape + (long long)e * sys.shape_stride + D.shape_off;
        const int o = (gy + D.woy) * D.dim + gx0 + tx0 + D.wox;
        if (D.type == AOMARL_DM_PZT) {
          add4(ph, slot + o);
        } else {
          const float c0 = slot[0], c1 = slot[1];
          float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          add4(f, D.influ + 2 * o);
          add4(f + 4, D.influ + 2 * o + 4);
#pragma unroll
          for (int j = 0; j < 4; j++) ph[j] += c0 * f[2 * j] + c1 * f[2 * j + 1];
        }
      }
    }
  }
  add4(mk, sys.mpupil + gy * sys.n + gx0 + tx0);
}

// Persistent waves: block = 4 waves, wave w of block bx walks sub-apertures
// (bx*4 + w) + k * gridDim.x*4 of environment blockIdx.y; the phase of the NEXT sub-aperture is
// fetched into registers while the MFMAs of the current one run (hides the load latency chain).
template <bool FROM_BUF, bool NOISE, bool WRITE_CUBE>
__global__ __launch_bounds__(256) void k_wfs_spot(DevSys sys, DevState st, int env_begin,
                                                  int no_atmos, int no_dms, int do_cog) {
  __shared__ float sAr[4][16][17];
  __shared__ float sAi[4][16][17];
  __shared__ float2 sTw[128];                    // (cos, sin)(2 pi m / 128)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e = env_begin + blockIdx.y;
  if (threadIdx.x < 128) {
    float sn, cs;
    sincospif((float)threadIdx.x * (1.0f / 64.0f), &sn, &cs);
    sTw[threadIdx.x] = make_float2(cs, sn);
  }
  __syncthreads();                               // the only block-wide barrier
  const int q = lane >> 4, c = lane & 15;
  const int stride = gridDim.x * 4;
  int i = blockIdx.x * 4 + wv;
  if (i >= sys.nvalid) return;

  // ---- twiddles: idx = 4q + s (pixel), half-integer frequency k + 1/2 with k = c
  float Cc[4], Ss[4];                            // cos / sin(2 pi (2c+1)(4q+s) / 128)
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const float2 w = sTw[((4 * q + s) * (2 * c + 1)) & 127];
    Cc[s] = w.x; Ss[s] = w.y;
  }
  const int ty = lane >> 2, tx0 = (lane & 3) * 4;

  float ph[4], mk[4];
  spot_load<FROM_BUF>(sys, st, e, i, lane, no_atmos, no_dms, ph, mk);
  for (; i < sys.nvalid; i += stride) {
    // ---- stage 0: complex amplitude tile -> LDS (4 pixels per lane)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float t = ph[j] * sys.wfs_inv_lambda;          // revolutions (the half-pixel ramp is folded
                                                     // into the half-integer frequencies)
      t -= rintf(t);
      const float sn = __builtin_amdgcn_sinf(t), cs = __builtin_amdgcn_cosf(t);   // v_sin/v_cos
      sAr[wv][ty][tx0 + j] = mk[j] * cs;
      sAi[wv][ty][tx0 + j] = mk[j] * sn;
    }
    // ---- prefetch the next sub-aperture of this wave
    const int inext = i + stride;
    if (inext < sys.nvalid) spot_load<FROM_BUF>(sys, st, e, inext, lane, no_atmos, no_dms, ph, mk);
    __builtin_amdgcn_wave_barrier();

    spot_compute<NOISE, WRITE_CUBE>(sys, st, e, i, lane, wv, Cc, Ss, sAr, sAi, do_cog, sys.flux[i]);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------------------------------------
// Fast variant for the production layout: NL atmosphere layers, DMs = [stack array, tip-tilt],
// every offset an integer, atmosphere and DMs both seen.  All loads of a tile are independent
// (raw values land in separate registers, the sum is formed at first use), so one wait covers the
// whole prefetch and it overlaps the MFMA block of the previous sub-aperture.  Per-environment
// constants (ring origins, TT commands) are read once per wave.
// ---------------------------------------------------------------------------------------------
template <int NL>
struct SpotEnv {
  const float *lay[NL];
  int px0[NL], py0[NL], dim[NL];
  const float *pzt;
  int pzt_dim, pzt_ox, pzt_oy;
  const float *tt;
  int tt_dim, tt_ox, tt_oy;
  float c0, c1;
};

template <int NL>
struct SpotRaw {
  float L[NL][4];
  float P[4], T[8], M[4];
  float F;   // fluxPerSub of the sub-aperture
};

// All loads of one tile.  Addresses are  uniform base pointer (SGPR) + 32-bit lane offset, so
// the compiler emits global_load ... v_off, s[base] with no 64-bit VALU arithmetic; ring wraps
// cost one v_sub + v_min_u32 per axis (px, px - dim as unsigned: the smaller one is in range).
template <int NL>
__device__ __forceinline__ void spot_fetch(const DevSys &sys, const SpotEnv<NL> &E, int xy0, int ty,
                                           int tx0, int i, SpotRaw<NL> &r) {
  const unsigned gx = (unsigned)((xy0 & 0xFFFF) + tx0), gy = (unsigned)((xy0 >> 16) + ty);
  r.F = sys.flux[i];
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const unsigned dim = (unsigned)E.dim[l];
    unsigned py = gy + (unsigned)E.py0[l]; py = min(py, py - dim);
    unsigned px = gx + (unsigned)E.px0[l]; px = min(px, px - dim);
    const unsigned off = py * (dim + RING_PAD) + px;
    const f4u t = *reinterpret_cast<const f4u *>(E.lay[l] + off);
#pragma unroll
    for (int j = 0; j < 4; j++) r.L[l][j] = t.v[j];
  }
  {
    const unsigned off = (gy + (unsigned)E.pzt_oy) * (unsigned)E.pzt_dim + gx + (unsigned)E.pzt_ox;
    const f4u t = *reinterpret_cast<const f4u *>(E.pzt + off);
#pragma unroll
    for (int j = 0; j < 4; j++) r.P[j] = t.v[j];
  }
  {
    const unsigned off = 2u * ((gy + (unsigned)E.tt_oy) * (unsigned)E.tt_dim + gx + (unsigned)E.tt_ox);
    const f4u t0 = *reinterpret_cast<const f4u *>(E.tt + off);
    const f4u t1 = *reinterpret_cast<const f4u *>(E.tt + off + 4u);
#pragma unroll
    for (int j = 0; j < 4; j++) { r.T[j] = t0.v[j]; r.T[4 + j] = t1.v[j]; }
  }
  {
    const unsigned off = gy * (unsigned)sys.n + gx;
    const f4u t = *reinterpret_cast<const f4u *>(sys.mpupil + off);
#pragma unroll
    for (int j = 0; j < 4; j++) r.M[j] = t.v[j];
  }
}

// stage-1 MFMAs + T combinations of the tile in sAr/sAi (see spot_compute for the algebra)
__device__ __forceinline__ void spot_stage1(int lane, const float (&Cc)[4], const float (&Ss)[4],
                                            const float (*bAr)[17], const float (*bAi)[17],
                                            f32x4 (&Tr)[2], f32x4 (&Ti)[2]) {
  const int q = lane >> 4, c = lane & 15;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 PCr = z4, PCi = z4, PSr = z4, PSi = z4;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const float br = bAr[c][4 * q + s], bi = bAi[c][4 * q + s];
    PCr = mfma16(br, Cc[s], PCr);
    PCi = mfma16(bi, Cc[s], PCi);
    PSr = mfma16(br, Ss[s], PSr);
    PSi = mfma16(bi, Ss[s], PSi);
  }
  Tr[0] = PCr + PSi; Ti[0] = PCi - PSr;
  Tr[1] = PCr - PSi; Ti[1] = PCi + PSr;
}

// Software-pipelined fast kernel.  Per wave and iteration k (tile k of this wave):
//   R1  stage-1 MFMAs of tile k (LDS buffer k&1), T combinations
//   R2  stage-2 MFMAs of tile k  INTERLEAVED (sched_group_barrier) with independent work:
//         amplitude of tile k+1 (sum of the prefetched sources, sin/cos) -> LDS buffer (k+1)&1,
//         address arithmetic + issue of the loads of tile k+2
//   R3  X combinations, |X|^2, binning, COG, store of tile k
// so the VALU / VMEM / LDS-write work of the neighbouring tiles hides under the matrix pipe of
// the current one instead of serialising with it.  The loop body is one basic block (indices are
// clamped instead of branched on).
template <int NL, bool NOISE, bool WRITE_CUBE>
__global__ __launch_bounds__(256) void k_wfs_spot_fast(DevSys sys, DevState st, int env_begin,
                                                       int do_cog) {
  __shared__ float sAr[4][2][16][17];
  __shared__ float sAi[4][2][16][17];
  __shared__ float2 sTw[128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e = env_begin + blockIdx.y;
  if (threadIdx.x < 128) {
    float sn, cs;
    sincospif((float)threadIdx.x * (1.0f / 64.0f), &sn, &cs);
    sTw[threadIdx.x] = make_float2(cs, sn);
  }
  __syncthreads();
  const int q = lane >> 4, c = lane & 15;
  const int stride = gridDim.x * 4;
  const int i0 = blockIdx.x * 4 + wv;
  if (i0 >= sys.nvalid) return;
  const int nit = (sys.nvalid - i0 + stride - 1) / stride;      // tiles of this wave
  const int ilast = i0 + (nit - 1) * stride;
  float Cc[4], Ss[4];                            // cos / sin(2 pi (2c+1)(4q+s) / 128)
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const float2 w = sTw[((4 * q + s) * (2 * c + 1)) & 127];
    Cc[s] = w.x; Ss[s] = w.y;
  }
  const int ty = lane >> 2, tx0 = (lane & 3) * 4;
  const bool owner = (c & 1) == 0;
  // ---- per-environment constants
  SpotEnv<NL> E;
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const DevLayer &L = sys.layers[l];
    E.lay[l] = st.screens + (long long)e * sys.screen_stride + L.screen_off;
    E.dim[l] = L.dim;
    int px = L.wox + st.origin[(e * sys.nlayers + l) * 2]; px -= (px >= L.dim) ? L.dim : 0;
    int py = L.woy + st.origin[(e * sys.nlayers + l) * 2 + 1]; py -= (py >= L.dim) ? L.dim : 0;
    E.px0[l] = px; E.py0[l] = py;
  }
  {
    const DevDm &D0 = sys.dms[0], &D1 = sys.dms[1];
    E.pzt = st.dm_shape + (long long)e * sys.shape_stride + D0.shape_off;
    E.pzt_dim = D0.dim; E.pzt_ox = D0.wox; E.pzt_oy = D0.woy;
    const float *slot = st.dm_shape + (long long)e * sys.shape_stride + D1.shape_off;
    E.c0 = slot[0]; E.c1 = slot[1];
    E.tt = D1.influ; E.tt_dim = D1.dim; E.tt_ox = D1.wox; E.tt_oy = D1.woy;
  }
  const float inv_lambda = sys.wfs_inv_lambda;
  SpotRaw<NL> raw;
  auto amplitude_to_lds = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float ph = raw.P[j] + (E.c0 * raw.T[2 * j] + E.c1 * raw.T[2 * j + 1]);
#pragma unroll
      for (int l = 0; l < NL; l++) ph += raw.L[l][j];
      float t = ph * inv_lambda;
      t -= rintf(t);
      const float sn = __builtin_amdgcn_sinf(t), cs = __builtin_amdgcn_cosf(t);
      sAr[wv][buf][ty][tx0 + j] = raw.M[j] * cs;
      sAi[wv][buf][ty][tx0 + j] = raw.M[j] * sn;
    }
  };
  // ---- prologue: tile 0 -> LDS buffer 0, loads of tile 1 in flight
  spot_fetch<NL>(sys, E, sys.sub_xy[i0], ty, tx0, i0, raw);
  float flux_cur = raw.F;
  amplitude_to_lds(0);
  {
    const int i1 = min(i0 + stride, ilast);
    spot_fetch<NL>(sys, E, sys.sub_xy[i1], ty, tx0, i1, raw);
  }
  int xy2 = sys.sub_xy[min(i0 + 2 * stride, ilast)];
  __builtin_amdgcn_wave_barrier();

  for (int k = 0; k < nit; k++) {
    const int i = i0 + k * stride;
    const int buf = k & 1;
    // ---- R1
    f32x4 Tr[2], Ti[2];
    spot_stage1(lane, Cc, Ss, sAr[wv][buf], sAi[wv][buf], Tr, Ti);
    // ---- R2: stage-2 MFMAs ...
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 Xr[2][2], Xi[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
      f32x4 QCr = z4, QCi = z4, QSr = z4, QSi = z4;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        QCr = mfma16(Cc[s], Tr[m][s], QCr);
        QCi = mfma16(Cc[s], Ti[m][s], QCi);
        QSr = mfma16(Ss[s], Tr[m][s], QSr);
        QSi = mfma16(Ss[s], Ti[m][s], QSi);
      }
      Xr[0][m] = QCr + QSi; Xi[0][m] = QCi - QSr;
      Xr[1][m] = QCr - QSi; Xi[1][m] = QCi + QSr;
    }
    // ... with the neighbours' work: amplitude of tile k+1, loads of tile k+2
    const float flux_next = raw.F;
    amplitude_to_lds(buf ^ 1);
    {
      const int i2 = min(i + 2 * stride, ilast);
      spot_fetch<NL>(sys, E, xy2, ty, tx0, i2, raw);
      xy2 = sys.sub_xy[min(i + 3 * stride, ilast)];
    }
#pragma unroll
    for (int r = 0; r < 32; r++) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // 1 MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);     // 5 VALU
      __builtin_amdgcn_sched_group_barrier(0x220, 1, 0);     // 1 VMEM read or DS write
    }
    // ---- R3: |X|^2, 2x2 binning, flux / COG, store (same mapping as spot_compute)
    float v[2][2][2];
    float tot = 0.f;
#pragma unroll
    for (int sy = 0; sy < 2; sy++)
#pragma unroll
      for (int sx = 0; sx < 2; sx++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
          float a0 = Xr[sy][sx][2 * h], b0 = Xi[sy][sx][2 * h];
          float a1 = Xr[sy][sx][2 * h + 1], b1 = Xi[sy][sx][2 * h + 1];
          float t = (a0 * a0 + b0 * b0) + (a1 * a1 + b1 * b1);
          t = add_xor1(t);
          v[sy][sx][h] = t;
          tot += t;
        }
    const int Xp = 8 + (c >> 1), Xm = 7 - (c >> 1);
    float *sl = st.slopes + (long long)e * sys.nslope;
    if (!NOISE && !WRITE_CUBE) {
      float sx_ = 0.f, sy_ = 0.f;
#pragma unroll
      for (int sy = 0; sy < 2; sy++)
#pragma unroll
        for (int sx = 0; sx < 2; sx++)
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const int Y = sy ? 7 - (2 * q + h) : 8 + 2 * q + h;
            sx_ += v[sy][sx][h] * (float)(sx ? Xm : Xp);
            sy_ += v[sy][sx][h] * (float)Y;
          }
      tot = wave_sum(owner ? tot : 0.f);
      sx_ = wave_sum(owner ? sx_ : 0.f);
      sy_ = wave_sum(owner ? sy_ : 0.f);
      if (do_cog && lane == 0) {
        const float inv = tot > 0.f ? 1.0f / tot : 0.f;
        sl[i] = tot > 0.f ? (sx_ * inv - sys.cog_offset) * sys.cog_scale : 0.f;
        sl[sys.nvalid + i] = tot > 0.f ? (sy_ * inv - sys.cog_offset) * sys.cog_scale : 0.f;
      }
    } else {
      tot = wave_sum(owner ? tot : 0.f);
      const float g = tot > 0.f ? sys.nphot * flux_cur / tot : 0.f;
      float s0 = 0.f, sx = 0.f, sy = 0.f;
      if (NOISE) {
        // lane parity h takes pixel h of each (ty, tx) of the pair's 8 pixels (see spot_finish)
        const int hh = c & 1;
        const uint32_t sd = st.seeds[e], fr = st.frame[e];
#pragma unroll
        for (int ty_ = 0; ty_ < 2; ty_++)
#pragma unroll
          for (int tx_ = 0; tx_ < 2; tx_++) {
            const int Y = ty_ ? 7 - (2 * q + hh) : 8 + 2 * q + hh, X = tx_ ? Xm : Xp;
            const uint32_t idx = (uint32_t)i * 256u + (uint32_t)(Y * 16 + X);
            const float val = sh_noise((hh ? v[ty_][tx_][1] : v[ty_][tx_][0]) * g, sys.noise, sd, fr, idx);
            if (WRITE_CUBE) st.bincube[((long long)e * sys.nvalid + i) * 256 + Y * 16 + X] = val;
            s0 += val;
            sx += val * (float)X;
            sy += val * (float)Y;
          }
      } else {
#pragma unroll
        for (int ty_ = 0; ty_ < 2; ty_++)
#pragma unroll
          for (int tx_ = 0; tx_ < 2; tx_++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
              const int Y = ty_ ? 7 - (2 * q + h) : 8 + 2 * q + h, X = tx_ ? Xm : Xp;
              const float val = v[ty_][tx_][h] * g;
              if (WRITE_CUBE && owner)
                st.bincube[((long long)e * sys.nvalid + i) * 256 + Y * 16 + X] = val;
              s0 += val;
              sx += val * (float)X;
              sy += val * (float)Y;
            }
      }
      if (do_cog) {
        s0 = wave_sum((NOISE || owner) ? s0 : 0.f);
        sx = wave_sum((NOISE || owner) ? sx : 0.f);
        sy = wave_sum((NOISE || owner) ? sy : 0.f);
        if (lane == 0) {
          sl[i] = s0 != 0.f ? (sx / s0 - sys.cog_offset) * sys.cog_scale : 0.f;
          sl[sys.nvalid + i] = s0 != 0.f ? (sy / s0 - sys.cog_offset) * sys.cog_scale : 0.f;
        }
      }
    }
    flux_cur = flux_next;
    __builtin_amdgcn_wave_barrier();
  }
}

// (the one-pass frame kernel, k_frame_wave: aomarl_frame.hip)

// COG from a stored bincube (Rtc.do_centroids on its own): one wave per sub-aperture
__global__ __launch_bounds__(256) void k_cog(DevSys sys, DevState st, int env_begin) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv;
  const int e = env_begin + blockIdx.y;
  if (i >= sys.nvalid) return;
  const int np2 = sys.npix * sys.npix;
  const float *im = st.bincube + ((long long)e * sys.nvalid + i) * np2;
  float s0 = 0.f, sx = 0.f, sy = 0.f;
  for (int p = lane; p < np2; p += 64) {
    float val = im[p];
    int y = p / sys.npix, x = p - y * sys.npix;
    s0 += val; sx += val * (float)x; sy += val * (float)y;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s0 += __shfl_xor(s0, o); sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o);
  }
  if (lane == 0) {
    float *sl = st.slopes + (long long)e * sys.nslope;
    if (s0 != 0.f) {
      sl[i] = (sx / s0 - sys.cog_offset) * sys.cog_scale;
      sl[sys.nvalid + i] = (sy / s0 - sys.cog_offset) * sys.cog_scale;
    } else {
      sl[i] = 0.f; sl[sys.nvalid + i] = 0.f;
    }
  }
}

// geometric slopes from st->wfs_phase (calibration only): one wave per sub-aperture
__global__ __launch_bounds__(256) void k_slopes_geom(DevSys sys, DevState st, int env_begin) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv;
  const int e = env_begin + blockIdx.y;
  if (i >= sys.nvalid) return;
  const int pd = sys.pdiam, n = sys.n;
  const int xy0 = sys.sub_xy[i];
  const int gx0 = xy0 & 0xFFFF, gy0 = xy0 >> 16;
  const float *ph = st.wfs_phase + (long long)e * n * n;
  float gx = 0.f, gyv = 0.f;
  for (int k = lane; k < pd * pd; k += 64) {
    int y = k / pd, x = k - y * pd;
    int xm = x > 0 ? x - 1 : x, xp = x < pd - 1 ? x + 1 : x;
    int ym = y > 0 ? y - 1 : y, yp = y < pd - 1 ? y + 1 : y;
    float m = sys.mpupil[(gy0 + y) * n + gx0 + x];
    float dx = (ph[(gy0 + y) * n + gx0 + xp] - ph[(gy0 + y) * n + gx0 + xm]) / (float)(xp - xm);
    float dy = (ph[(gy0 + yp) * n + gx0 + x] - ph[(gy0 + ym) * n + gx0 + x]) / (float)(yp - ym);
    gx += m * dx; gyv += m * dy;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { gx += __shfl_xor(gx, o); gyv += __shfl_xor(gyv, o); }
  if (lane == 0) {
    const float alpha = 0.206265f / sys.subapd;
    const float den = (float)pd * sys.flux[i];
    float *sl = st.slopes + (long long)e * sys.nslope;
    sl[i] = alpha * gx / den;
    sl[sys.nvalid + i] = alpha * gyv / den;
  }
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

// =============================================================================================
// science target: fused raytrace + windowed PSF (separable DFT) + phase variance
// stage 1: R[y][kx] = sum_x a(y, x) exp(-2 pi i kx x / Npsf), kx in [-hw, hw)
// =============================================================================================
#define TGT_XC 64
template <bool FROM_BUF>
__global__ __launch_bounds__(256) void k_target_rows(DevSys sys, DevState st, int env_begin,
                                                     float *__restrict__ TR,
                                                     float *__restrict__ TPART, int nblk) {
  extern __shared__ float smem[];
  const int W = 2 * sys.hw, RB = 256 / W, pd = sys.pupdiam, np = sys.npsf;
  float *sar = smem;                      // [RB][TGT_XC]
  float *sai = sar + RB * TGT_XC;
  float *red = sai + RB * TGT_XC;         // [3][256]
  float2 *stw = reinterpret_cast<float2 *>(red + 3 * 256);   // [np] (only if it fits)
  const bool tw_lds = np <= 4096;
  const int tid = threadIdx.x;
  const int e = env_begin + blockIdx.y;
  const int y0 = blockIdx.x * RB;
  const float2 *gtw = reinterpret_cast<const float2 *>(sys.psf_tw);
  if (tw_lds)
    for (int j = tid; j < np; j += 256) stw[j] = gtw[j];
  const float2 *tw = tw_lds ? stw : gtw;
  // pivot for the variance sums: phase at the pupil-grid centre
  float pivot;
  {
    const int cx = pd / 2, cy = pd / 2;
    float v = 0.f;
    if (FROM_BUF) {
      v = st.tar_phase[(long long)e * pd * pd + cy * pd + cx];
    } else {
      for (int l = 0; l < sys.nlayers; l++) {
        const DevLayer &L = sys.layers[l];
        const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
        const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
        v += base[ring_idx(cx + L.tox, cy + L.toy, ox, oy, L.dim)];
      }
      for (int k = 0; k < sys.ndm; k++)
        v += dm_value(sys, st, e, k, cx + sys.dms[k].tox, cy + sys.dms[k].toy);
    }
    pivot = v;
  }
  const int kxi = tid % W, ys = tid / W;
  const int kxf = kxi - sys.hw;
  float accr = 0.f, acci = 0.f;
  float sd = 0.f, sd2 = 0.f, sm = 0.f;
  for (int x0 = 0; x0 < pd; x0 += TGT_XC) {
    __syncthreads();
    for (int p = tid; p < RB * TGT_XC; p += 256) {
      const int yy = p / TGT_XC, xx = p - yy * TGT_XC;
      const int y = y0 + yy, x = x0 + xx;
      float ar = 0.f, ai = 0.f;
      if (y < pd && x < pd) {
        const float m = sys.spupil[y * pd + x];
        if (m != 0.f) {
          float v = 0.f;
          if (FROM_BUF) {
            v = st.tar_phase[(long long)e * pd * pd + y * pd + x];
          } else {
            for (int l = 0; l < sys.nlayers; l++) {
              const DevLayer &L = sys.layers[l];
              const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
              const int ox = st.origin[(e * sys.nlayers + l) * 2];
              const int oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
              v += base[ring_idx(x + L.tox, y + L.toy, ox, oy, L.dim)];
            }
            for (int k = 0; k < sys.ndm; k++)
              v += dm_value(sys, st, e, k, x + sys.dms[k].tox, y + sys.dms[k].toy);
          }
          float t = v * sys.tar_inv_lambda;
          t -= rintf(t);
          float sn, cs;
          sincospif(2.0f * t, &sn, &cs);
          ar = m * cs; ai = m * sn;
          const float d = v - pivot;
          sd += d; sd2 += d * d; sm += 1.f;
        }
      }
      sar[p] = ar; sai[p] = ai;
    }
    __syncthreads();
    if (ys < RB) {
      const int xmax = (pd - x0) < TGT_XC ? (pd - x0) : TGT_XC;
      for (int xx = 0; xx < xmax; xx++) {
        const float ar = sar[ys * TGT_XC + xx], ai = sai[ys * TGT_XC + xx];
        const float2 w = tw[(kxf * (x0 + xx)) & (np - 1)];   // (cos, sin); e^{-i t} = cos - i sin
        accr += ar * w.x + ai * w.y;
        acci += ai * w.x - ar * w.y;
      }
    }
  }
  if (ys < RB && y0 + ys < pd) {
    float *o = TR + (((long long)blockIdx.y * pd + (y0 + ys)) * W + kxi) * 2;
    o[0] = accr; o[1] = acci;
  }
  // block partial sums for the variance
  red[tid] = sd; red[256 + tid] = sd2; red[512 + tid] = sm;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; red[512 + tid] += red[512 + tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float *pp = TPART + ((long long)blockIdx.y * nblk + blockIdx.x) * 4;
    pp[0] = red[0]; pp[1] = red[256]; pp[2] = red[512]; pp[3] = 0.f;
  }
}

// (the sinc fit of the PSF peak -- sinc_gain, fit_axis_gain, psf_window_fit: aomarl_trace_dev.h)

// stage 2: G[ky][kx] = sum_y R[y][kx] exp(-2 pi i ky y / Npsf); |G|^2 -> pending window;
// variance from the block partials -> pending[W*W]
__global__ __launch_bounds__(256) void k_target_finish(DevSys sys, const float *__restrict__ TR,
                                                       const float *__restrict__ TPART, int nblk,
                                                       float *__restrict__ PEND) {
  const int W = 2 * sys.hw, pd = sys.pupdiam, np = sys.npsf;
  const int b = blockIdx.x;     // env within the batch
  const float2 *tw = reinterpret_cast<const float2 *>(sys.psf_tw);
  const float2 *R = reinterpret_cast<const float2 *>(TR) + (long long)b * pd * W;
  float *pend = PEND + (long long)b * (W * W + 4);
  for (int o = threadIdx.x; o < W * W; o += blockDim.x) {
    const int ky = o / W, kx = o - ky * W;
    const int kyf = ky - sys.hw;
    float gr = 0.f, gi = 0.f;
    for (int y = 0; y < pd; y++) {
      const float2 r = R[y * W + kx];
      const float2 w = tw[(kyf * y) & (np - 1)];
      gr += r.x * w.x + r.y * w.y;
      gi += r.y * w.x - r.x * w.y;
    }
    pend[o] = gr * gr + gi * gi;
  }
  __syncthreads();
  psf_window_fit(pend, W);
  if (threadIdx.x == 0) {
    double sd = 0., sd2 = 0., sm = 0.;
    for (int k = 0; k < nblk; k++) {
      const float *pp = TPART + ((long long)b * nblk + k) * 4;
      sd += pp[0]; sd2 += pp[1]; sm += pp[2];
    }
    double var = 0.;
    if (sm > 0.) { double mean = sd / sm; var = sd2 / sm - mean * mean; }
    pend[W * W] = (float)var;
  }
}


// ---------------------------------------------------------------------------------------------
// MFMA version (hw == 8 -> 16 kept frequencies per axis = one 16-wide MFMA tile).
// Block = 16 pupil rows; the complex amplitude of a 16 x 64 chunk is staged in LDS; the 4 waves
// split the chunk's 64 columns (K) and accumulate R[16 y][16 kx] with v_mfma_f32_16x16x4_f32:
//   Rr += ar*C + ai*S ; Ri += ai*C - ar*S ,  C/S[x][kx] = cos/sin(2 pi kx x / Npsf)
// ---------------------------------------------------------------------------------------------
template <bool FROM_BUF>
__global__ __launch_bounds__(256) void k_target_rows_mfma(DevSys sys, DevState st, int env_begin,
                                                          float *__restrict__ TR,
                                                          float *__restrict__ TPART, int nblk) {
  extern __shared__ float smem[];
  const int pd = sys.pupdiam, np = sys.npsf;
  float *sar = smem;                       // [16][65]
  float *sai = sar + 16 * 65;
  float *red = sai + 16 * 65;              // [4 waves][2][256] partial tiles; reused for sums
  float2 *stw = reinterpret_cast<float2 *>(red + 4 * 2 * 256);   // [np] if it fits
  const bool tw_lds = np <= 4096;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, c = lane & 15;
  const int e = env_begin + blockIdx.y;
  const int y0 = blockIdx.x * 16;
  const float2 *gtw = reinterpret_cast<const float2 *>(sys.psf_tw);
  if (tw_lds)
    for (int j = tid; j < np; j += 256) stw[j] = gtw[j];
  const float2 *tw = tw_lds ? stw : gtw;
  float pivot;
  {
    const int cx = pd / 2, cy = pd / 2;
    float v = 0.f;
    if (FROM_BUF) {
      v = st.tar_phase[(long long)e * pd * pd + cy * pd + cx];
    } else {
      for (int l = 0; l < sys.nlayers; l++) {
        const DevLayer &L = sys.layers[l];
        const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
        const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
        v += base[ring_idx(cx + L.tox, cy + L.toy, ox, oy, L.dim)];
      }
      for (int k = 0; k < sys.ndm; k++)
        v += dm_value(sys, st, e, k, cx + sys.dms[k].tox, cy + sys.dms[k].toy);
    }
    pivot = v;
  }
  f32x4 Rr = {0.f, 0.f, 0.f, 0.f}, Ri = {0.f, 0.f, 0.f, 0.f};
  float sd = 0.f, sd2 = 0.f, sm = 0.f;
  const int fy = tid >> 4, fx0 = (tid & 15) * 4;     // fill: row fy, 4 consecutive columns
  const int y = y0 + fy;
  const int kxf = c - 8;
  for (int x0 = 0; x0 < pd; x0 += 64) {
    __syncthreads();
    {
      float ph[4] = {0.f, 0.f, 0.f, 0.f};
      float mk[4] = {0.f, 0.f, 0.f, 0.f};
      const int xb = x0 + fx0;
      if (y < pd) {
        // pd % 4 == 0 (checked at create): a group of 4 columns is entirely inside or outside
        if (xb < pd) add4(mk, sys.spupil + y * pd + xb);
        if (FROM_BUF) {
          if (xb < pd) add4(ph, st.tar_phase + (long long)e * pd * pd + y * pd + xb);
        } else if (xb < pd) {
          for (int l = 0; l < sys.nlayers; l++) {
            const DevLayer &L = sys.layers[l];
            const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
            const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
            int py = y + L.toy + oy; py -= (py >= L.dim) ? L.dim : 0;
            int px = xb + L.tox + ox; px -= (px >= L.dim) ? L.dim : 0;
            add4_ring(ph, base + py * (L.dim + RING_PAD), px, L.dim);
          }
          for (int k = 0; k < sys.ndm; k++) {
            const DevDm &D = sys.dms[k];
            const float *slot = st.dm_shape + (long long)e * sys.shape_stride + D.shape_off;
            const int o = (y + D.toy) * D.dim + xb + D.tox;
            if (D.type == AOMARL_DM_PZT) {
              add4(ph, slot + o);
            } else {
              const float c0 = slot[0], c1 = slot[1];
              float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              add4(f, D.influ + 2 * o);
              add4(f + 4, D.influ + 2 * o + 4);
#pragma unroll
              for (int j = 0; j < 4; j++) ph[j] += c0 * f[2 * j] + c1 * f[2 * j + 1];
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float ar = 0.f, ai = 0.f;
        if (mk[j] != 0.f) {
          float t = ph[j] * sys.tar_inv_lambda;
          t -= rintf(t);
          ar = mk[j] * __builtin_amdgcn_cosf(t);
          ai = mk[j] * __builtin_amdgcn_sinf(t);
          const float d = ph[j] - pivot;
          sd += d; sd2 += d * d; sm += 1.f;
        }
        sar[fy * 65 + fx0 + j] = ar;
        sai[fy * 65 + fx0 + j] = ai;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int xl = 16 * wv + 4 * s + q;
      const float ar = sar[c * 65 + xl], ai = sai[c * 65 + xl];
      const float2 w = tw[(kxf * (x0 + xl)) & (np - 1)];
      Rr = mfma16(ar, w.x, Rr);
      Ri = mfma16(ai, w.x, Ri);
      Rr = mfma16(ai, w.y, Rr);
      Ri = mfma16(ar, -w.y, Ri);
    }
  }
  __syncthreads();
  // cross-wave reduction of the 4 partial tiles; acc reg r of lane (q, c): y = 4q + r, kx = c
#pragma unroll
  for (int r = 0; r < 4; r++) {
    red[(wv * 2 + 0) * 256 + (4 * q + r) * 16 + c] = Rr[r];
    red[(wv * 2 + 1) * 256 + (4 * q + r) * 16 + c] = Ri[r];
  }
  __syncthreads();
  {
    const int yy = tid >> 4, kx = tid & 15;
    if (y0 + yy < pd) {
      float vr = 0.f, vi = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < 4; w4++) { vr += red[(w4 * 2) * 256 + tid]; vi += red[(w4 * 2 + 1) * 256 + tid]; }
      float *o = TR + (((long long)blockIdx.y * pd + (y0 + yy)) * 16 + kx) * 2;
      o[0] = vr; o[1] = vi;
    }
  }
  __syncthreads();
  red[tid] = sd; red[256 + tid] = sd2; red[512 + tid] = sm;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; red[512 + tid] += red[512 + tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float *pp = TPART + ((long long)blockIdx.y * nblk + blockIdx.x) * 4;
    pp[0] = red[0]; pp[1] = red[256]; pp[2] = red[512]; pp[3] = 0.f;
  }
}

// Fast variant (production layout: NL layers, DMs = [stack array, tip-tilt], integer offsets):
// per-environment constants hoisted, all loads of a chunk independent and issued one chunk ahead
// of their use (software pipeline), double-buffered LDS tile -> one barrier per chunk.
template <int NL>
__global__ __launch_bounds__(256) void k_target_rows_fast(DevSys sys, DevState st, int env_begin,
                                                          float *__restrict__ TR,
                                                          float *__restrict__ TPART, int nblk) {
  extern __shared__ float smem[];
  const int pd = sys.pupdiam, np = sys.npsf;
  float *sar = smem;                       // [2][16][65]
  float *sai = sar + 2 * 16 * 65;
  float *red = sai + 2 * 16 * 65;          // [4 waves][2][256]
  float2 *stw = reinterpret_cast<float2 *>(red + 4 * 2 * 256);
  const bool tw_lds = np <= 4096;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, c = lane & 15;
  const int e = env_begin + blockIdx.y;
  const int y0 = blockIdx.x * 16;
  const float2 *gtw = reinterpret_cast<const float2 *>(sys.psf_tw);
  if (tw_lds)
    for (int j = tid; j < np; j += 256) stw[j] = gtw[j];
  const float2 *tw = tw_lds ? stw : gtw;
  // ---- per-environment constants
  const float *lay[NL];
  int lpx[NL], lpy[NL], ldim[NL];
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const DevLayer &L = sys.layers[l];
    lay[l] = st.screens + (long long)e * sys.screen_stride + L.screen_off;
    ldim[l] = L.dim;
    int px = L.tox + st.origin[(e * sys.nlayers + l) * 2]; px -= (px >= L.dim) ? L.dim : 0;
    int py = L.toy + st.origin[(e * sys.nlayers + l) * 2 + 1]; py -= (py >= L.dim) ? L.dim : 0;
    lpx[l] = px; lpy[l] = py;
  }
  const DevDm &D0 = sys.dms[0], &D1 = sys.dms[1];
  const float *pzt = st.dm_shape + (long long)e * sys.shape_stride + D0.shape_off;
  const float *ttslot = st.dm_shape + (long long)e * sys.shape_stride + D1.shape_off;
  const float c0 = ttslot[0], c1 = ttslot[1];
  const int fy = tid >> 4, fx0 = (tid & 15) * 4;
  const int y = y0 + fy;
  const bool row_ok = y < pd;
  // pivot of the variance sums: phase at the grid centre
  float pivot;
  {
    const int cx = pd / 2, cy = pd / 2;
    float v = pzt[(cy + D0.toy) * D0.dim + cx + D0.tox];
    const float2 f = reinterpret_cast<const float2 *>(D1.influ)[(cy + D1.toy) * D1.dim + cx + D1.tox];
    v += c0 * f.x + c1 * f.y;
#pragma unroll
    for (int l = 0; l < NL; l++) {
      int py = cy + lpy[l]; py -= (py >= ldim[l]) ? ldim[l] : 0;
      int px = cx + lpx[l]; px -= (px >= ldim[l]) ? ldim[l] : 0;
      v += lay[l][py * (ldim[l] + RING_PAD) + px];
    }
    pivot = v;
  }
  // row pointers of this thread
  const float *lrow[NL];
#pragma unroll
  for (int l = 0; l < NL; l++) {
    int py = (row_ok ? y : 0) + lpy[l]; py -= (py >= ldim[l]) ? ldim[l] : 0;
    lrow[l] = lay[l] + py * (ldim[l] + RING_PAD);
  }
  const float *prow = pzt + ((row_ok ? y : 0) + D0.toy) * D0.dim + D0.tox;
  const float *trow = D1.influ + 2 * (((row_ok ? y : 0) + D1.toy) * D1.dim + D1.tox);
  const float *mrow = sys.spupil + (row_ok ? y : 0) * pd;

  float rL[NL][4], rP[4], rT[8], rM[4];
  auto fetch = [&](int x0) {
    const int xb = x0 + fx0;
    const bool ok = row_ok && xb < pd;        // pd % 4 == 0: the 4 columns are in or out together
    const int xs = ok ? xb : 0;
#pragma unroll
    for (int l = 0; l < NL; l++) {
      int px = xs + lpx[l]; px -= (px >= ldim[l]) ? ldim[l] : 0;
      const f4u t = *reinterpret_cast<const f4u *>(lrow[l] + px);
#pragma unroll
      for (int j = 0; j < 4; j++) rL[l][j] = t.v[j];
    }
    const f4u tp = *reinterpret_cast<const f4u *>(prow + xs);
    const f4u t0 = *reinterpret_cast<const f4u *>(trow + 2 * xs);
    const f4u t1 = *reinterpret_cast<const f4u *>(trow + 2 * xs + 4);
    const f4u tm = *reinterpret_cast<const f4u *>(mrow + xs);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      rP[j] = tp.v[j]; rT[j] = t0.v[j]; rT[4 + j] = t1.v[j];
      rM[j] = ok ? tm.v[j] : 0.f;
    }
  };

  f32x4 Rr = {0.f, 0.f, 0.f, 0.f}, Ri = {0.f, 0.f, 0.f, 0.f};
  float sd = 0.f, sd2 = 0.f, sm = 0.f;
  const int kxf = c - 8;
  fetch(0);
  int buf = 0;
  for (int x0 = 0; x0 < pd; x0 += 64, buf ^= 1) {
    float *bar = sar + buf * 16 * 65, *bai = sai + buf * 16 * 65;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float ph = rP[j] + (c0 * rT[2 * j] + c1 * rT[2 * j + 1]);
#pragma unroll
      for (int l = 0; l < NL; l++) ph += rL[l][j];
      float ar = 0.f, ai = 0.f;
      if (rM[j] != 0.f) {
        float t = ph * sys.tar_inv_lambda;
        t -= rintf(t);
        ar = rM[j] * __builtin_amdgcn_cosf(t);
        ai = rM[j] * __builtin_amdgcn_sinf(t);
        const float d = ph - pivot;
        sd += d; sd2 += d * d; sm += 1.f;
      }
      bar[fy * 65 + fx0 + j] = ar;
      bai[fy * 65 + fx0 + j] = ai;
    }
    if (x0 + 64 < pd) fetch(x0 + 64);       // next chunk's loads fly during the barrier + MFMAs
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int xl = 16 * wv + 4 * s + q;
      const float ar = bar[c * 65 + xl], ai = bai[c * 65 + xl];
      const float2 w = tw[(kxf * (x0 + xl)) & (np - 1)];
      Rr = mfma16(ar, w.x, Rr);
      Ri = mfma16(ai, w.x, Ri);
      Rr = mfma16(ai, w.y, Rr);
      Ri = mfma16(ar, -w.y, Ri);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; r++) {
    red[(wv * 2 + 0) * 256 + (4 * q + r) * 16 + c] = Rr[r];
    red[(wv * 2 + 1) * 256 + (4 * q + r) * 16 + c] = Ri[r];
  }
  __syncthreads();
  {
    const int yy = tid >> 4, kx = tid & 15;
    if (y0 + yy < pd) {
      float vr = 0.f, vi = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < 4; w4++) { vr += red[(w4 * 2) * 256 + tid]; vi += red[(w4 * 2 + 1) * 256 + tid]; }
      float *o = TR + (((long long)blockIdx.y * pd + (y0 + yy)) * 16 + kx) * 2;
      o[0] = vr; o[1] = vi;
    }
  }
  __syncthreads();
  red[tid] = sd; red[256 + tid] = sd2; red[512 + tid] = sm;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; red[512 + tid] += red[512 + tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float *pp = TPART + ((long long)blockIdx.y * nblk + blockIdx.x) * 4;
    pp[0] = red[0]; pp[1] = red[256]; pp[2] = red[512]; pp[3] = 0.f;
  }
}

// stage 2 on MFMA: G[ky][kx] = sum_y E[ky][y] R[y][kx]; 4 waves split y, one block per env
__global__ __launch_bounds__(256) void k_target_finish_mfma(DevSys sys, const float *__restrict__ TR,
                                                            const float *__restrict__ TPART, int nblk,
                                                            float *__restrict__ PEND,
                                                            uint32_t *__restrict__ frame) {
  __shared__ float red[4 * 2 * 256];
  __shared__ double dred[3][64];
  const int pd = sys.pupdiam, np = sys.npsf;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, c = lane & 15;
  const float2 *tw = reinterpret_cast<const float2 *>(sys.psf_tw);
  const float2 *R = reinterpret_cast<const float2 *>(TR) + (long long)b * pd * 16;
  float *pend = PEND + (long long)b * (256 + 4);
  const int kyf = c - 8;
  f32x4 Gr = {0.f, 0.f, 0.f, 0.f}, Gi = {0.f, 0.f, 0.f, 0.f};
  const int per = ((pd + 15) / 16) * 4;              // rows per wave, multiple of 4
  const int yb = wv * per, ye = min(pd, yb + per);
  // 8 steps (32 rows) of operands are fetched before their MFMAs: the loop is latency-bound
  for (int y0 = yb; y0 < ye; y0 += 32) {
    float2 r[8], w[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int y = y0 + 4 * u + q;
      r[u] = make_float2(0.f, 0.f); w[u] = make_float2(0.f, 0.f);
      if (y < ye) {
        r[u] = R[y * 16 + c];                          // B operand: R[y][kx = c]
        w[u] = tw[(kyf * y) & (np - 1)];               // A operand: E[ky = c - 8][y]
      }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      Gr = mfma16(w[u].x, r[u].x, Gr);
      Gi = mfma16(w[u].x, r[u].y, Gi);
      Gr = mfma16(w[u].y, r[u].y, Gr);
      Gi = mfma16(-w[u].y, r[u].x, Gi);
    }
  }
#pragma unroll
  for (int r4 = 0; r4 < 4; r4++) {
    red[(wv * 2 + 0) * 256 + (4 * q + r4) * 16 + c] = Gr[r4];
    red[(wv * 2 + 1) * 256 + (4 * q + r4) * 16 + c] = Gi[r4];
  }
  if (tid < 64) {
    double sd = 0., sd2 = 0., sm = 0.;
    for (int k = tid; k < nblk; k += 64) {
      const float *pp = TPART + ((long long)b * nblk + k) * 4;
      sd += pp[0]; sd2 += pp[1]; sm += pp[2];
    }
    dred[0][tid] = sd; dred[1][tid] = sd2; dred[2][tid] = sm;
  }
  __syncthreads();
  {
    float gr = 0.f, gi = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < 4; w4++) { gr += red[(w4 * 2) * 256 + tid]; gi += red[(w4 * 2 + 1) * 256 + tid]; }
    pend[tid] = gr * gr + gi * gi;                     // tid = ky * 16 + kx
  }
  __syncthreads();
  psf_window_fit(pend, 16);
  if (tid == 0) {
    double sd = 0., sd2 = 0., sm = 0.;
    for (int k = 0; k < 64; k++) { sd += dred[0][k]; sd2 += dred[1][k]; sm += dred[2][k]; }
    double var = 0.;
    if (sm > 0.) { double mean = sd / sm; var = sd2 / sm - mean * mean; }
    pend[256] = (float)var;
    if (frame) frame[b] += 1u;                         // WFS noise frame counter (one-pass path)
  }
}

// publish the pending PSF (strehl_commit_body: aomarl_trace_dev.h)
__global__ __launch_bounds__(256) void k_strehl_commit(DevSys sys, DevState st, int env_begin,
                                                       const float *__restrict__ PEND) {
  strehl_commit_body(sys, st, env_begin, blockIdx.x, PEND);
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

// comp_strehl(do_fit = True), long exposure: the fitted peak of the accumulated window -> slot 7 (on demand:
// aomarl_strehl_fit; one wave per environment)
__global__ __launch_bounds__(64) void k_strehl_fit_le(DevSys sys, DevState st, int env_begin) {
  __shared__ float g2[4];
  const int W = 2 * sys.hw, e = env_begin + blockIdx.x, lane = threadIdx.x;
  float *le = st.le_img + (long long)e * W * W;
  float m = -1.f;
  int arg = 0;
  for (int o = lane; o < W * W; o += 64) { const float v = le[o]; if (v > m) { m = v; arg = o; } }
  for (int d = 32; d >= 1; d >>= 1) {
    const float m2 = __shfl_xor(m, d);
    const int a2 = __shfl_xor(arg, d);
    if (m2 > m || (m2 == m && a2 < arg)) { m = m2; arg = a2; }
  }
  if (lane < 2) g2[lane] = fit_axis_gain(le, W, arg, lane);
  __syncthreads();
  if (lane == 0) {
    float *s = st.strehl + (long long)e * 8;
    s[7] = s[4] > 0.f ? m * g2[0] * g2[1] / s[4] / sys.ref_peak : 0.f;
  }
}

__global__ void k_strehl_reset(DevSys sys, DevState st, int env_begin) {
  const int W = 2 * sys.hw;
  const int e = env_begin + blockIdx.x;
  for (int o = threadIdx.x; o < W * W; o += blockDim.x) st.le_img[(long long)e * W * W + o] = 0.f;
  if (threadIdx.x < 8) st.strehl[(long long)e * 8 + threadIdx.x] = 0.f;
}
