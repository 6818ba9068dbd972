// gemm_p_host_check.cpp -- a stand-alone host program around aomarl_gemm_p_host.h (k_gemm_p's tile menu, k split and
// pick) and aomarl_gemm_plan_host.h (launch_gemm_nt's plan: kernel, tile and k split of every product).  No GPU, no HIP:
//     g++ -std=c++17 -O2 -o gemm_p_host_check gemm_p_host_check.cpp
// (by hand also with -g -fsanitize=address,undefined -fno-sanitize-recover=all).  It walks gemm_p_pick over
// M, N in {1, 31, 32, 33, 64, 127, 128, 129, 256, 768, 1286}, every K in 1 .. 4100, max_split in {1, 16} and a
// workspace of 0, 1, 3 and 16 products, and requires of every configuration what k_gemm_p relies on:
//   kchunk % 32 == 0;  1 <= nz <= max_split;  (nz - 1) kchunk < K <= nz kchunk (every chunk non-empty);
//   the tile is on the menu;  nz == 1 without a workspace or with max_split == 1;  nz M N <= ws_floats when nz > 1;
//   tiles_m x tiles_n block tiles cover M x N, and no tile row / column lies wholly outside.
// gemm_p_chunks is checked on its own for every K and every asked split 1 .. 20, and K = 0 (no chunk, no
// configuration, no division by zero).
// Then gemm_plan over the same M, N plus 63 and 65, every K in 1 .. 4100, operands aligned or not, a workspace of 0, 1, 3
// and 16 products, fast x the "gemm_split_f16" option, "gemm_target_blocks" in {0, 256, 512}, min_chunk in {128, 288} and
// pick_M in {0, M / 4, M}, and requires of every plan what the three kernels and the reduces rely on:
//   aligned and not split-f16: k_gemm_p with exactly gemm_p_pick(Mp, N, K, the part's share, ws ? 16 : 1), tiles_m for M;
//   unaligned: k_gemm_nt, kchunk % 32 == 0;  split-f16: k_gemm_nt_h, kchunk % 96 == 0;
//   (nz - 1) kchunk < K <= nz kchunk;  nz == 1 without a workspace;  nz M N <= ws_floats when nz > 1 (the real M);
//   pick_M = m gives the tile, nz and kchunk of a product of m rows with its share of the workspace;
//   the fallback behind k_gemm_p (gemm_plan_fallback) obeys the same rules with kchunk % 96 == 0;
//   K <= 0: no plan and no refusal;  every refusal of a forced value comes back with its text.
// Exit status 0: all held.  (The grid is 388 876 800 plans: 145 828 800 k_gemm_p, 194 438 400 k_gemm_nt, 48 609 600
// k_gemm_nt_h.)  With --plans: nothing of the above, one line per production shape instead (the k_gemm_p
// section) at 8, 64, 256 and 768 rows, aligned and not, a workspace of 0 / 4 / 16 products, both min_chunk values, and
// the fast mode off and on -- which here means the "gemm_split_f16" option: every loop call site passes fast = true,
// so GemmQuery::fast is true in every line.  tests/golden/gemm_plans.txt pins them, so that a cost-model change that
// moves one shows.
#include "aomarl_gemm_plan_host.h"
#include <stdio.h>
#include <string.h>

#define REQUIRE(c)                                                                                          \
  do {                                                                                                      \
    if (!(c)) {                                                                                             \
      fprintf(stderr, "%s:%d: %s failed (M %d N %d K %d max_split %d ws %zu -> wm %d wn %d nz %d kchunk %d " \
                      "tiles %d x %d)\n", __FILE__, __LINE__, #c, M, N, K, ms, ws, c_.wm, c_.wn, c_.nz,     \
              c_.kchunk, c_.tiles_m, c_.tiles_n);                                                           \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

static const GemmOptions opt0 = {/* xcd */ 1, /* target_blocks */ 0, /* split_f16 */ false};

static const char *kernel_name(int k) { return k == GEMM_P ? "k_gemm_p" : k == GEMM_NT ? "k_gemm_nt" : k == GEMM_NT_H ? "k_gemm_nt_h" : "none"; }

static int print_plans() {
  static const struct { const char *name; int N, K; } shapes[] = {
      {"extrusion_40x40", 648, 1957}, {"do_control_40x40", 1286, 2400}, {"v2m_40x40", 1283, 1286}, {"m2v_40x40", 1286, 1283},
      {"shortcut_40x40", 1283, 2400}, {"extrusion_10x10", 168, 513},    {"do_control_10x10", 88, 128}, {"v2m_10x10", 87, 88},
      {"m2v_10x10", 88, 87},          {"shortcut_10x10", 87, 128}};
  static const int rows[] = {8, 64, 256, 768}, wsm[] = {0, 4, 16}, mcs[] = {128, 288};
  for (const auto &s : shapes)
    for (int M : rows)
      for (int al = 1; al >= 0; al--)
        for (int w : wsm)
          for (int mc : mcs)
            for (int sp = 0; sp < 2; sp++) {
              GemmOptions opt = opt0;
              opt.split_f16 = sp != 0;
              const GemmQuery q = {M, s.N, s.K, al != 0, (size_t)w * M * s.N, /* fast */ true, mc, /* pick_M */ 0};
              const GemmPlan p = gemm_plan(q, opt, nullptr);
              const bool isp = p.kernel == GEMM_P;
              const int bm = isp ? 32 * p.p.wm : 64, bn = isp ? 32 * p.p.wn : 64;
              printf("%s M=%d N=%d K=%d aligned=%d ws=%d min_chunk=%d split_f16=%d : %s tile=%dx%d tiles=%dx%d nz=%d kchunk=%d\n", s.name, M,
                     s.N, s.K, al, w, mc, sp, kernel_name(p.kernel), bm, bn, (M + bm - 1) / bm, (s.N + bn - 1) / bn,
                     isp ? p.p.nz : p.nz, isp ? p.p.kchunk : p.kchunk);
            }
  return 0;
}

#define PREQ(c)                                                                                                   \
  do {                                                                                                            \
    if (!(c)) {                                                                                                   \
      fprintf(stderr, "%s:%d: %s failed (M %d N %d K %d aligned %d ws %zu fast %d min_chunk %d pick_M %d; split_f16 %d "  \
                      "target_blocks %d -> kernel %d, k_gemm_p %d x %d nz %d kchunk %d tiles %d x %d, 64 x 64 nz %d kchunk %d)\n",  \
              __FILE__, __LINE__, #c, q.M, q.N, q.K, (int)q.aligned, q.ws_floats, (int)q.fast, q.min_chunk, q.pick_M,   \
              (int)opt.split_f16, opt.target_blocks, p.kernel, p.p.wm, p.p.wn, p.p.nz, p.p.kchunk, p.p.tiles_m,    \
              p.p.tiles_n, p.nz, p.kchunk);                                                                        \
      return false;                                                                                               \
    }                                                                                                             \
  } while (0)

// what every k split must satisfy, whichever kernel runs it: chunks of whole k-tiles (mult: 32, or 96 where the kernel
// walks groups of three), every chunk non-empty, the slabs inside the workspace
static bool split_holds(const GemmQuery &q, const GemmOptions &opt, const GemmPlan &p, int nz, int kchunk, int mult) {
  PREQ(p.error == nullptr);
  PREQ(p.xcd == opt.xcd);
  PREQ(kchunk > 0 && kchunk % mult == 0);
  PREQ(nz >= 1 && (long long)(nz - 1) * kchunk < q.K && q.K <= (long long)nz * kchunk);
  if (q.ws_floats == 0) PREQ(nz == 1);
  if (nz > 1) PREQ((size_t)nz * q.M * q.N <= q.ws_floats);
  return true;
}

// what every plan must satisfy (p: the plan of q under opt; w: gemm_p_pick for q's shape)
static bool plan_holds(const GemmQuery &q, const GemmOptions &opt, const GemmPlan &p, const GemmPCfg &w) {
  const bool split = q.aligned && q.fast && opt.split_f16;
  PREQ(p.kernel == (!q.aligned ? GEMM_NT : split ? GEMM_NT_H : GEMM_P));
  if (p.kernel != GEMM_P) return split_holds(q, opt, p, p.nz, p.kchunk, p.kernel == GEMM_NT_H ? 96 : 32);
  if (!split_holds(q, opt, p, p.p.nz, p.p.kchunk, 32)) return false;
  PREQ(p.p.wm == w.wm && p.p.wn == w.wn && p.p.nz == w.nz && p.p.kchunk == w.kchunk && p.p.tiles_n == w.tiles_n);
  PREQ(p.p.wm > 0 && p.p.tiles_m == (q.M + 32 * p.p.wm - 1) / (32 * p.p.wm));
  return true;
}

static const char *refusal(int M, int N, int K, bool al, size_t ws, GemmForceIn f) {
  const GemmQuery q = {M, N, K, al, ws, false, 128, 0};
  const GemmPlan p = gemm_plan(q, opt0, &f);
  return p.kernel == GEMM_NONE && p.error ? p.error : "";
}

static int walk_plans() {
  static const int dims[] = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 768, 1286};
  static const int wsmul[] = {0, 1, 3, 16}, tbs[] = {0, 256, 512}, mcs[] = {128, 288};
  const int nd = (int)(sizeof(dims) / sizeof(dims[0]));
  long long plans = 0, by_kernel[4] = {0, 0, 0, 0}, split = 0;
  for (int im = 0; im < nd; im++)
    for (int in = 0; in < nd; in++) {
      const int M = dims[im], N = dims[in];
      for (int K = 1; K <= 4100; K++)
        for (int iw = 0; iw < 4; iw++)
          for (int ip = 0; ip < 3; ip++) {
            const int pick_M = ip == 0 ? 0 : ip == 1 ? M / 4 : M;
            if (ip == 1 && pick_M < 1) continue;
            const size_t ws = (size_t)wsmul[iw] * M * N;
            const int Mp = pick_M > 0 ? pick_M : M;
            const GemmPCfg want = gemm_p_pick(Mp, N, K, pick_M > 0 ? (size_t)((double)ws * Mp / M) : ws, ws ? 16 : 1);
            // (the axes the k_gemm_p pick does not depend on go innermost: its memo then answers all but the first)
            for (int al = 0; al < 2; al++)
              for (int fs = 0; fs < 4; fs++)
                for (int it = 0; it < 3; it++)
                  for (int ic = 0; ic < 2; ic++) {
                    const GemmOptions opt = {1, tbs[it], (fs & 2) != 0};
                    const GemmQuery q = {M, N, K, al != 0, ws, (fs & 1) != 0, mcs[ic], pick_M};
                    GemmPlan p = gemm_plan(q, opt, nullptr);
                    if (!plan_holds(q, opt, p, want)) return 1;
                    plans++; by_kernel[p.kernel]++;
                    split += (p.kernel == GEMM_P ? p.p.nz : p.nz) > 1;
                    if (pick_M > 0) {            // the part on its own, with its share of the workspace
                      const GemmQuery qm = {pick_M, N, K, al != 0, (size_t)wsmul[iw] * pick_M * N, (fs & 1) != 0, mcs[ic], 0};
                      const GemmPlan m = gemm_plan(qm, opt, nullptr);
                      if (!(m.kernel == p.kernel && m.p.wm == p.p.wm && m.p.wn == p.p.wn && m.p.nz == p.p.nz &&
                            m.p.kchunk == p.p.kchunk && m.nz == p.nz && m.kchunk == p.kchunk)) {
                        fprintf(stderr, "gemm_p_host_check: M %d N %d K %d with pick_M %d is not planned as %d rows are\n", M, N, K, pick_M, pick_M);
                        return 1;
                      }
                    }
                    if (p.kernel == GEMM_P) {    // where k_gemm_p cannot be launched: k_gemm_nt, whole groups of three k-tiles
                      gemm_plan_fallback(q, opt, nullptr, &p);
                      if (p.kernel != GEMM_NT || !split_holds(q, opt, p, p.nz, p.kchunk, 96)) { fprintf(stderr, "gemm_p_host_check: the fallback plan of M %d N %d K %d\n", M, N, K); return 1; }
                    }
                  }
          }
    }
  // K <= 0 and empty shapes: no plan, no refusal, no trap
  static const int empty[][3] = {{5, 5, 0}, {5, 5, -1}, {0, 5, 5}, {5, 0, 5}, {-2, 5, 5}, {0, 0, 0}};
  for (const auto &e : empty)
    for (int al = 0; al < 2; al++)
      for (int w = 0; w < 2; w++) {
        const GemmQuery q = {e[0], e[1], e[2], al != 0, (size_t)w * 4096, true, 128, w ? 3 : 0};
        const GemmForceIn f = {w, 0, 0, al, 0};
        const GemmPlan a = gemm_plan(q, opt0, nullptr), b = gemm_plan(q, opt0, &f);
        if (a.kernel != GEMM_NONE || a.error || b.kernel != GEMM_NONE || b.error) {
          fprintf(stderr, "gemm_p_host_check: a plan or a refusal for the empty product %d x %d x %d\n", e[0], e[1], e[2]);
          return 1;
        }
      }
  // the refusals of forced values, each with its text
  const size_t big = (size_t)16 * 64 * 64;
  const struct { const char *got, *want; } refusals[] = {
      {refusal(64, 64, 256, false, big, GemmForceIn{1, 0, 0, 0, 0}), "kernel / wm / wn (operands not 16-byte aligned)"},
      {refusal(64, 64, 256, false, big, GemmForceIn{3, 0, 0, 0, 0}), "kernel / wm / wn (operands not 16-byte aligned)"},
      {refusal(64, 64, 256, false, big, GemmForceIn{0, 2, 2, 0, 0}), "kernel / wm / wn (operands not 16-byte aligned)"},
      {refusal(64, 64, 256, true, big, GemmForceIn{0, 3, 4, 0, 0}), "wm / wn (not an instantiated tile)"},
      {refusal(64, 64, 256, true, big, GemmForceIn{1, 2, 0, 0, 0}), "wm / wn (not an instantiated tile)"},
      {refusal(64, 64, 256, true, big, GemmForceIn{2, 2, 2, 0, 0}), "wm / wn (k_gemm_p only)"},
      {refusal(64, 64, 256, true, big, GemmForceIn{3, 2, 2, 0, 0}), "wm / wn (k_gemm_p only)"},
      {refusal(64, 64, 256, true, 0, GemmForceIn{0, 0, 0, 2, 0}), "ksplit (no workspace)"},
      {refusal(64, 64, 256, false, 0, GemmForceIn{2, 0, 0, 3, 0}), "ksplit (no workspace)"},
      {refusal(64, 64, 256, true, big, GemmForceIn{0, 0, 0, -1, 0}), "ksplit (no workspace)"},
      {refusal(64, 64, 256, true, 2 * 64 * 64, GemmForceIn{1, 0, 0, 3, 0}), "ksplit (the slabs do not fit work_floats)"},
      {refusal(64, 64, 256, true, 2 * 64 * 64, GemmForceIn{2, 0, 0, 3, 0}), "ksplit (the slabs do not fit work_floats)"},
      {refusal(64, 64, 576, true, 2 * 64 * 64, GemmForceIn{3, 0, 0, 3, 0}), "ksplit (the slabs do not fit work_floats)"},
      {refusal(64, 64, 256, true, big, GemmForceIn{1, 4, 4, 3, 2}), ""},      // and what can be had is not refused
      {refusal(64, 64, 256, false, big, GemmForceIn{2, 0, 0, 3, 1}), ""},
  };
  for (const auto &r : refusals)
    if (strcmp(r.got, r.want)) {
      fprintf(stderr, "gemm_p_host_check: refusal \"%s\" where \"%s\" was due\n", r.got, r.want);
      return 1;
    }
  if (!by_kernel[GEMM_P] || !by_kernel[GEMM_NT] || !by_kernel[GEMM_NT_H] || !split) {
    fprintf(stderr, "gemm_p_host_check: a kernel was never planned, or nothing was split\n");
    return 1;
  }
  printf("gemm_plan: ok (%lld plans: %lld k_gemm_p, %lld k_gemm_nt, %lld k_gemm_nt_h; %lld of them split)\n", plans, by_kernel[GEMM_P],
         by_kernel[GEMM_NT], by_kernel[GEMM_NT_H], split);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--plans")) return print_plans();
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
  return walk_plans();
}
