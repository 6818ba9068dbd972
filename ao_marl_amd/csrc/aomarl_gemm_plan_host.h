// aomarl_gemm_plan_host.h -- what launch_gemm_nt (aomarl_gemm_nt.h) decides before it launches anything: which of the
// three kernels takes a product C = alpha A . B^T, and with which tile and k split.  No HIP include and no global: the
// process-wide options come in as an argument, so the stand-alone host program (gemm_p_host_check.cpp) walks the same
// text over a grid of shapes, also under the address and undefined-behaviour sanitizers.
#pragma once
#include "aomarl_gemm_p_host.h"

struct GemmOptions {     // process-wide (aomarl_set_option / aomarl_set_precision); a call may pass a changed copy
  int xcd;               // "gemm_xcd_map": k_gemm_nt_h's / k_gemm_p's blocks grouped by k-chunk per XCD
  int target_blocks;     // "gemm_target_blocks": 0: the 64 x 64 kernels' split-K by the blocks-per-CU cost model; > 0: about that many blocks
  bool split_f16;        // "gemm_split_f16": the internal GEMMs (extrusion, command matrix, Btt projections) on k_gemm_nt_h
};

struct GemmQuery {
  int M, N, K;
  bool aligned;          // both operands 16-byte aligned with leading dimensions that are multiples of 4
  size_t ws_floats;      // the split-K workspace (0: none, never split)
  bool fast;             // the split-f16 kernel may be used (internal call sites whose operands are inside its range)
  int min_chunk;         // the 64 x 64 kernels' shortest k-chunk
  int pick_M;            // > 0: tile and split-K as a product of pick_M rows would get them (a sum's order depends on the k
                         //      split alone: M rows at once then give, bit for bit, what M / pick_M products of pick_M rows give)
};

// aomarl_gemm_nt_probe's wishes (tests only; null everywhere else).  A forced value that cannot be had is refused
// (GemmPlan::error names the argument), never replaced.
struct GemmForceIn {
  int kernel;            // 0 = the library's choice, 1 = k_gemm_p, 2 = k_gemm_nt (also on aligned operands), 3 = k_gemm_nt_h
  int wm, wn;            // k_gemm_p's tile (both or neither)
  int ksplit;            // k-chunks asked for
  int xcd;               // 0 = the "gemm_xcd_map" option, 1 = on, 2 = off
};

enum { GEMM_NONE = 0, GEMM_P = 1, GEMM_NT = 2, GEMM_NT_H = 3 };        // (GemmForceIn::kernel's numbers)

struct GemmPlan {
  int kernel;            // GEMM_NONE: an empty product, or refused (error)
  GemmPCfg p;            // GEMM_P: k_gemm_p's configuration, tiles_m for the real M
  int nz, kchunk;        // GEMM_NT / GEMM_NT_H: the 64 x 64 kernels' k-chunks and their length
  int xcd;
  const char *error;     // null, or what was refused
  GemmPCfg pick;         // with a GemmForceIn: gemm_p_pick for this shape and workspace, computed afresh beside the memo (wm == 0: k_gemm_p not considered)
};

// The 64 x 64 kernels' k split (al: whole groups of three k-tiles, as k_gemm_nt_h's gh_mainloop wants them).
static inline void gemm_plan_64(const GemmQuery &q, const GemmOptions &opt, const GemmForceIn *force, bool al,
                                GemmPlan *p) {
  const int M = q.M, N = q.N, K = q.K, min_chunk = q.min_chunk;
  const int Mp = q.pick_M > 0 ? q.pick_M : M;
  const size_t wsp = q.pick_M > 0 ? (size_t)((double)q.ws_floats * Mp / M) : q.ws_floats;     // the part's share of the workspace
  const int bx = (N + 63) / 64, byp = (Mp + 63) / 64;
  int nsplit = 1;
  if (q.ws_floats > 0 && bx * byp < 384) {
    // Split K so that the launch is as short as its slowest CU: blocks go round-robin over the 256 CUs, a CU
    // that gets one block more than the others sets the duration (528 blocks = 2.06 per CU took as long as 768
    // would: 132 tiles x 4 chunks lost to 132 x 3 = 396).  Cost model per candidate: blocks per CU (rounded
    // up) x k-tiles per block (whole groups of three for the pipelined kernels, + 2 tiles of fill / drain).
    // min_chunk: the control chain's products ask for at least three groups of three k-tiles per block
    // (288): below that the fill / drain of the load pipeline and the wider reduce cost more than the
    // extra blocks bring (round-2 script gemm_split_time.py, since removed).
    const int ncu = 256, tiles = bx * byp;
    if (opt.target_blocks > 0) {                 // "gemm_target_blocks" > 0: the plain rule (about that many blocks)
      nsplit = (opt.target_blocks + tiles - 1) / tiles;
      if (nsplit > 8) nsplit = 8;
      while (nsplit > 1 && (K / nsplit < min_chunk || (size_t)nsplit * Mp * N > wsp)) nsplit--;
    } else {
      long long best = -1;
      for (int ns = 1; ns <= 8; ns++) {
        if (ns > 1 && (K / ns < min_chunk || (size_t)ns * Mp * N > wsp)) break;
        const int chunk = al ? ((K + ns - 1) / ns + 95) / 96 * 96 : (((K + ns - 1) / ns + 31) & ~31);
        const int nz = (K + chunk - 1) / chunk;
        const long long per_cu = ((long long)tiles * nz + ncu - 1) / ncu;
        const long long cost = per_cu * (chunk / 32 + 3);
        if (best < 0 || cost < best) { best = cost; nsplit = ns; }
      }
    }
  }
  if (force && force->ksplit) nsplit = force->ksplit;
  int kchunk = ((K + nsplit - 1) / nsplit + 31) & ~31;
  if (al) kchunk = ((K + nsplit - 1) / nsplit + 95) / 96 * 96;
  nsplit = (K + kchunk - 1) / kchunk;
  if (force && force->ksplit && nsplit > 1 && (size_t)nsplit * M * N > q.ws_floats) {
    p->kernel = GEMM_NONE;
    p->error = "ksplit (the slabs do not fit work_floats)";
    return;
  }
  p->nz = nsplit; p->kchunk = kchunk;
}

static inline GemmPlan gemm_plan(const GemmQuery &q, const GemmOptions &opt, const GemmForceIn *force) {
  GemmPlan p = {GEMM_NONE, {0, 0, 0, 0, 0, 0}, 0, 0, 0, nullptr, {0, 0, 0, 0, 0, 0}};
  const int M = q.M, N = q.N, K = q.K;
  if (M <= 0 || N <= 0 || K <= 0) return p;      // (an empty sum: the entry points refuse K == 0, no internal product has one)
  const bool ws = q.ws_floats > 0;
  bool al = q.aligned;
  if (force) {
    if ((force->kernel == 1 || force->kernel == 3 || force->wm || force->wn) && !al) { p.error = "kernel / wm / wn (operands not 16-byte aligned)"; return p; }
    if ((force->wm || force->wn) && !gemm_p_on_menu(force->wm, force->wn)) { p.error = "wm / wn (not an instantiated tile)"; return p; }
    if ((force->wm || force->wn) && force->kernel != 0 && force->kernel != 1) { p.error = "wm / wn (k_gemm_p only)"; return p; }
    if (force->ksplit < 0 || (force->ksplit > 1 && !ws)) { p.error = "ksplit (no workspace)"; return p; }
    if (force->kernel == 2) al = false;          // the element-wise kernel on aligned operands
  }
  p.xcd = force && force->xcd ? (force->xcd == 1 ? 1 : 0) : opt.xcd;
  const bool split_f16 = al && ((q.fast && opt.split_f16) || (force && force->kernel == 3));
  if (!al || split_f16) {
    p.kernel = split_f16 ? GEMM_NT_H : GEMM_NT;
    gemm_plan_64(q, opt, force, al, &p);
    return p;
  }
  // the balanced kernel; tile and k split from its own cost model (memoised per shape)
  const int Mp = q.pick_M > 0 ? q.pick_M : M;
  const size_t wsf = q.pick_M > 0 ? (size_t)((double)q.ws_floats * Mp / M) : q.ws_floats;     // the part's share of the workspace
  struct Memo { int M, N, K; size_t ws; GemmPCfg c; };
  static thread_local Memo memo[16];
  static thread_local int memo_n = 0;
  const GemmPCfg *cfg = nullptr;
  GemmPCfg fresh;
  if (force) {                                   // a probe call reports the pick computed afresh
    p.pick = fresh = gemm_p_pick(Mp, N, K, wsf, ws ? 16 : 1);
    if (force->wm || force->ksplit) cfg = &fresh;            // forced: the memo is neither read nor written
  }
  for (int i = 0; i < memo_n && !cfg; i++)
    if (memo[i].M == Mp && memo[i].N == N && memo[i].K == K && memo[i].ws == wsf) { cfg = &memo[i].c; break; }
  if (!cfg) {
    Memo &m = memo[memo_n < 16 ? memo_n++ : (memo_n = 1, 0)];
    m.M = Mp; m.N = N; m.K = K; m.ws = wsf;
    m.c = gemm_p_pick(Mp, N, K, wsf, ws ? 16 : 1);
    cfg = &m.c;
  }
  p.p = *cfg;                                    // (pick_M: the part's tile and k split over this product's rows)
  if (force && (force->wm || force->ksplit)) {   // forced tile and / or k split: the other one stays the pick's
    gemm_p_cost(Mp, N, K, force->wm ? force->wm : p.p.wm, force->wm ? force->wn : p.p.wn,
                force->ksplit ? force->ksplit : p.p.nz, &p.p);
    if (p.p.nz > 1 && (size_t)p.p.nz * M * N > q.ws_floats) { p.error = "ksplit (the slabs do not fit work_floats)"; return p; }
  }
  if (p.p.wm > 0) p.p.tiles_m = (M + 32 * p.p.wm - 1) / (32 * p.p.wm);
  p.kernel = GEMM_P;
  return p;
}

// k_gemm_p could not be launched: the product goes to k_gemm_nt with the 64 x 64 kernels' own split
static inline void gemm_plan_fallback(const GemmQuery &q, const GemmOptions &opt, const GemmForceIn *force, GemmPlan *p) {
  p->kernel = GEMM_NT;
  gemm_plan_64(q, opt, force, true, p);
}
