// aomarl_gemm_p_host.h -- the host side of k_gemm_p's configuration (aomarl_gemm_p.h): the tile menu, the k split into
// chunks, the cost model and the pick.  No HIP include: the library takes it through aomarl_gemm_p.h, and a
// stand-alone host program (gemm_p_host_check.cpp) walks it over a grid of shapes, also under the address and
// undefined-behaviour sanitizers.
#pragma once
#include <cstddef>

#define GP_KT 32          // k-tile

struct GemmPCfg {
  int wm, wn;            // wave tile in 16-granules; block tile = (32 wm) x (32 wn)
  int nz, kchunk;        // k-chunks and their length (a multiple of GP_KT)
  int tiles_m, tiles_n;
};

// the instantiations the library carries
#define GP_FOR_EACH_TILE(X) X(4, 4) X(4, 3) X(4, 2) X(2, 4) X(2, 3) X(2, 2) X(3, 3) X(3, 2)

static inline bool gemm_p_on_menu(int wm, int wn) {
#define GP_IS(a, b) if (wm == a && wn == b) return true;
  GP_FOR_EACH_TILE(GP_IS)
#undef GP_IS
  return false;
}

// kchunk for a split into (about) ns chunks: whole k-tiles, every chunk non-empty (K <= 0: no chunk at all, nz = 0 --
// gemm_p_pick then returns no configuration, wm == 0)
static inline void gemm_p_chunks(int K, int ns, int *kchunk, int *nz) {
  const int kt = K > 0 ? (K + GP_KT - 1) / GP_KT : 0;
  const int per = kt > 0 ? (kt + (ns > 1 ? ns : 1) - 1) / (ns > 1 ? ns : 1) : 1;
  *kchunk = per * GP_KT;
  *nz = (kt + per - 1) / per;
}

// Cost model (cycles of the busiest SIMD, roughly): workgroups go round-robin over ncu CUs, two of them share a
// CU's four SIMDs.  Per workgroup: k-tiles x (8 wm wn matrix instructions x 32 cycles + a barrier's skew) + fill
// + the tile's stores; plus what the consumer pays for reading nz slabs.
static inline double gemm_p_cost(int M, int N, int K, int wm, int wn, int ns, GemmPCfg *out) {
  const int ncu = 256;
  const int BM = 32 * wm, BN = 32 * wn;
  GemmPCfg c;
  c.wm = wm; c.wn = wn;
  c.tiles_m = (M + BM - 1) / BM; c.tiles_n = (N + BN - 1) / BN;
  gemm_p_chunks(K, ns, &c.kchunk, &c.nz);
  const long long G = (long long)c.tiles_m * c.tiles_n * c.nz;
  const long long per_cu = (G + ncu - 1) / ncu;
  const double ktile = 8.0 * wm * wn * 32.0 + 250.0;
  const double wg = (c.kchunk / GP_KT) * ktile + 2500.0 + 16.0 * wm * wn * 4.0;
  // slabs: written once, read once by the consumer (~4 B/clk/CU effective each way)
  const double slabs = c.nz > 1 ? 2.0 * c.nz * (double)M * N * 4.0 / (ncu * 8.0) : 0.0;
  if (out) *out = c;
  return per_cu * wg + slabs;
}

static inline GemmPCfg gemm_p_pick(int M, int N, int K, size_t ws_floats, int max_split) {
  GemmPCfg best = {0, 0, 0, 0, 0, 0};
  double bc = -1.0;
#define GP_TRY(a, b)                                                                      \
  for (int ns = 1; ns <= max_split; ns++) {                                               \
    GemmPCfg c;                                                                           \
    const double cost = gemm_p_cost(M, N, K, a, b, ns, &c);                               \
    if (c.nz > 1 && (size_t)c.nz * M * N > ws_floats) break;                              \
    if (c.nz < ns) continue;                                                              \
    if (bc < 0 || cost < bc) { bc = cost; best = c; }                                     \
  }
  GP_FOR_EACH_TILE(GP_TRY)
#undef GP_TRY
  return best;
}
