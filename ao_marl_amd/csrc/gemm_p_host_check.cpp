// gemm_p_host_check.cpp -- a stand-alone host program around aomarl_gemm_p_host.h (k_gemm_p's tile menu, k split and
// pick).  No GPU, no HIP:
//     g++ -std=c++17 -O2 -o gemm_p_host_check gemm_p_host_check.cpp
// (by hand also with -g -fsanitize=address,undefined -fno-sanitize-recover=all).  It walks gemm_p_pick over
// M, N in {1, 31, 32, 33, 64, 127, 128, 129, 256, 768, 1286}, every K in 1 .. 4100, max_split in {1, 16} and a
// workspace of 0, 1, 3 and 16 products, and requires of every configuration what k_gemm_p relies on:
//   kchunk % 32 == 0;  1 <= nz <= max_split;  (nz - 1) kchunk < K <= nz kchunk (every chunk non-empty);
//   the tile is on the menu;  nz == 1 without a workspace or with max_split == 1;  nz M N <= ws_floats when nz > 1;
//   tiles_m x tiles_n block tiles cover M x N, and no tile row / column lies wholly outside.
// gemm_p_chunks is checked on its own for every K and every asked split 1 .. 20, and K = 0 (no chunk, no
// configuration, no division by zero).  Exit status 0: all held.
#include "aomarl_gemm_p_host.h"
#include <stdio.h>

#define REQUIRE(c)                                                                                          \
  do {                                                                                                      \
    if (!(c)) {                                                                                             \
      fprintf(stderr, "%s:%d: %s failed (M %d N %d K %d max_split %d ws %zu -> wm %d wn %d nz %d kchunk %d " \
                      "tiles %d x %d)\n", __FILE__, __LINE__, #c, M, N, K, ms, ws, c_.wm, c_.wn, c_.nz,     \
              c_.kchunk, c_.tiles_m, c_.tiles_n);                                                           \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

int main() {
  static const int dims[] = {1, 31, 32, 33, 64, 127, 128, 129, 256, 768, 1286};
  static const int splits[] = {1, 16};
  static const int wsmul[] = {0, 1, 3, 16};
  const int nd = (int)(sizeof(dims) / sizeof(dims[0]));
  long long checked = 0, split_cfgs = 0;

  // the menu itself
  int menu = 0;
  for (int wm = 0; wm <= 8; wm++)
    for (int wn = 0; wn <= 8; wn++) menu += gemm_p_on_menu(wm, wn) ? 1 : 0;
  if (menu != 8 || gemm_p_on_menu(0, 0) || gemm_p_on_menu(3, 4) || !gemm_p_on_menu(3, 2)) {
    fprintf(stderr, "gemm_p_host_check: the tile menu has %d entries\n", menu);
    return 1;
  }

  // the k split alone: whole k-tiles, every chunk non-empty, never more chunks than asked for
  for (int K = 1; K <= 4100; K++)
    for (int ns = 1; ns <= 20; ns++) {
      int kchunk = -1, nz = -1;
      gemm_p_chunks(K, ns, &kchunk, &nz);
      if (kchunk <= 0 || kchunk % GP_KT || nz < 1 || nz > ns || (long long)(nz - 1) * kchunk >= K ||
          (long long)nz * kchunk < K) {
        fprintf(stderr, "gemm_p_host_check: gemm_p_chunks(K %d, ns %d) -> kchunk %d nz %d\n", K, ns, kchunk, nz);
        return 1;
      }
    }

  // K == 0 (an empty sum) has no chunk and no configuration; neither function may trap on it
  for (int ns = 0; ns <= 20; ns++) {
    int kchunk = -1, nz = -1;
    gemm_p_chunks(0, ns, &kchunk, &nz);
    if (nz != 0 || kchunk != GP_KT) {
      fprintf(stderr, "gemm_p_host_check: gemm_p_chunks(K 0, ns %d) -> kchunk %d nz %d\n", ns, kchunk, nz);
      return 1;
    }
  }
  for (int im = 0; im < nd; im++)
    for (int is = 0; is < 2; is++) {
      const GemmPCfg z = gemm_p_pick(dims[im], dims[nd - 1 - im], 0, (size_t)16 * dims[im] * dims[nd - 1 - im], splits[is]);
      if (z.wm != 0 || z.nz != 0) {
        fprintf(stderr, "gemm_p_host_check: gemm_p_pick with K 0 returned a configuration (wm %d nz %d)\n", z.wm, z.nz);
        return 1;
      }
    }

  for (int im = 0; im < nd; im++)
    for (int in = 0; in < nd; in++) {
      const int M = dims[im], N = dims[in];
      for (int K = 1; K <= 4100; K++)
        for (int is = 0; is < 2; is++)
          for (int iw = 0; iw < 4; iw++) {
            const int ms = splits[is];
            const size_t ws = (size_t)wsmul[iw] * M * N;
            const GemmPCfg c_ = gemm_p_pick(M, N, K, ws, ms);
            REQUIRE(gemm_p_on_menu(c_.wm, c_.wn));
            REQUIRE(c_.kchunk > 0 && c_.kchunk % 32 == 0);
            REQUIRE(c_.nz >= 1 && c_.nz <= ms);
            REQUIRE((long long)(c_.nz - 1) * c_.kchunk < K && K <= (long long)c_.nz * c_.kchunk);
            if (ws == 0 || ms == 1) REQUIRE(c_.nz == 1);
            if (c_.nz > 1) REQUIRE((size_t)c_.nz * M * N <= ws);
            REQUIRE(c_.tiles_m >= 1 && c_.tiles_n >= 1);
            REQUIRE((long long)c_.tiles_m * 32 * c_.wm >= M && (long long)(c_.tiles_m - 1) * 32 * c_.wm < M);
            REQUIRE((long long)c_.tiles_n * 32 * c_.wn >= N && (long long)(c_.tiles_n - 1) * 32 * c_.wn < N);
            checked++;
            split_cfgs += c_.nz > 1;
          }
    }
  if (split_cfgs == 0) {
    fprintf(stderr, "gemm_p_host_check: no shape was split at all\n");
    return 1;
  }
  printf("gemm_p_host_check: ok (%lld configurations, %lld of them split)\n", checked, split_cfgs);
  return 0;
}
