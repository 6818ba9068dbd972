// aomarl_move_plan_host.h -- what a move or a reset of the atmosphere (aomarl_capi_atmos.hip) decides before it launches
// anything: which environments move together, how a shift becomes rounds, which launches a round is, and in how many
// parts a reset walks its rounds.  No HIP include and no global: the facts come in as plain structs (atmos_facts in
// aomarl_capi_atmos.hip is the one place that reads them off the context), so the stand-alone host program
// (move_plan_host_check.cpp) walks the same text over every combination of them, also under the address and
// undefined-behaviour sanitizers; tests/golden/move_plans.txt pins the launch sequence.  The executor
// (ExtrudeRun::launch, move_atmos_now, aomarl_reset*) asks, then launches: it owns the streams, the events and the waits.
//
// The rules:
//
//   shift   per environment and layer, in float arithmetic: ax = accum + delta, k = (int)ax, accum = ax - (float)k
//           (x and y alike).  move_group is the only place that computes it.
//   group   a maximal run of consecutive environments with equal shifts: one launch sequence, its products over the
//           group's columns.  The whole batch is uniform (the graph step's key) exactly when its first group is all of it.
//   rounds  layer l queues |kx| x operations (dir +-1), then |ky| y operations (dir +-2); round r holds the r-th
//           operation of every layer that still has one, so the rounds thin out.  A reset: 2 dim operations per layer
//           along x with the sign of deltax -- on the transposed screen (dir +-2, tflag 1) unless "reset_untransposed".
//   round   one sub-round per [A|B] class with an operation in it, in class order: GATHER, PRODUCT, SCATTER.
//           SCATTER_GATHER replaces the scatter and the NEXT round's gather when the round is one sub-round, a next round
//           exists, holds layers of this round only (next_round) and of this class only, ns <= SG_U SG_THREADS,
//           dim <= SG_MAX_N and "extrude_unfused" is off; the next round then has no GATHER of its own, and works on the
//           other Z / ZREF pair: the parity flips there and nowhere else.
//   write   every scatter (and the small move) writes ring lines: is_write.  The executor orders those behind the
//           screens' readers.
//   ride    the plain SCATTER of the last class index in the last round may carry the caller's event on its dispatch
//           (may_ride); if that class has no operation in the last round, nothing rides.  The small move's one launch may.
//           Whether it does is the executor's: an event to carry, the whole batch, not capturing.
//   small   "small_move" and screens that fit k_move_small: the group's whole move is ONE launch, MOVE_SMALL.
//   overlap a move may run beside the OLDER frame in flight when every line it rewrites is outside the windows that frame
//           reads: kx <= tox (or -kx <= dim - tox - pupdiam), the same in y.  Asked only when such a frame exists.
//   complete every layer of the group moves (else nobody writes that ring's entry of the origin snapshot).
//   parts   a reset of n environments: min("reset_streams", 4) parts when that is > 1, "prefetch_atmos" is on, n >= 16 x
//           "reset_streams" and nothing is capturing, else one; part k of what is left: (b + n - e0) / (parts - k)
//           environments.  The prefetched reset with "reset_prefetch_whole": one range whose products take a part's tile
//           and k split (pick_n), when n divides.
#pragma once
#include "../../include/aomarl.h"      // AOMARL_MAX_LAYERS

// k_extrude_sg: longest line it keeps in LDS; threads per column; stencil items per thread (ns <= SG_U * SG_THREADS)
constexpr int SG_MAX_N = 1024, SG_THREADS = 512, SG_U = 4;
// k_move_small: ns + dim and dim it holds in LDS, its threads
constexpr int MOVE_SMALL_K = 4096, MOVE_SMALL_DIM = 256, MOVE_SMALL_T = 512;

// ---- kernel arguments
struct RoundOps {
  int nops;
  int layer[AOMARL_MAX_LAYERS];
  int dir[AOMARL_MAX_LAYERS];
  int tflag[AOMARL_MAX_LAYERS];     // 1: the screen holds the transpose (reset): dir is +-2, stencil istT
};
// the round behind a round, as the fused scatter + gather sees it: idx[i] = position of operation i's layer in the next
// round (-1: that layer is done), dir / tflag of the next round's operations
struct RoundNext {
  int nops;
  int idx[AOMARL_MAX_LAYERS];
  int dir[AOMARL_MAX_LAYERS];
  int tflag[AOMARL_MAX_LAYERS];
};
// signed pixel shifts per layer of one frame's move (k_move_small takes it as it is)
struct MoveShift { int kx[AOMARL_MAX_LAYERS], ky[AOMARL_MAX_LAYERS]; };

// ---- facts
struct AtmosFacts {
  int nlayers, nclass;
  int abclass[AOMARL_MAX_LAYERS], dim[AOMARL_MAX_LAYERS], ns[AOMARL_MAX_LAYERS];
  int tox[AOMARL_MAX_LAYERS], toy[AOMARL_MAX_LAYERS], pupdiam;      // the frame kernel's windows
  bool unfused;          // "extrude_unfused"
  bool small;            // "small_move" and every layer fits k_move_small
};

// ---- shifts and groups
struct MoveGroup {
  int b, n;              // environments [b, b + n)
  MoveShift k;
  float fx[AOMARL_MAX_LAYERS], fy[AOMARL_MAX_LAYERS];    // the remainders of environment b ("subpixel_flow" uses the range's first)
};

// The group that starts at environment e0 of [e0, end) (rows of nl accumulators).  remx / remy: where the group's
// remainders go -- the accumulators themselves (a move), or null (a question: nothing is written).
static inline MoveGroup move_group(int nl, const float *accumx, const float *accumy, float *remx, float *remy,
                                   const float *deltax, const float *deltay, int e0, int end) {
  MoveGroup g;
  g.b = e0;
  for (int l = 0; l < AOMARL_MAX_LAYERS; l++) { g.k.kx[l] = 0; g.k.ky[l] = 0; g.fx[l] = 0.f; g.fy[l] = 0.f; }
  int e = e0;
  for (; e < end; e++) {
    const size_t row = (size_t)e * nl;
    MoveShift k;
    float fx[AOMARL_MAX_LAYERS], fy[AOMARL_MAX_LAYERS];
    bool same = true;
    for (int l = 0; l < nl; l++) {
      const float ax = accumx[row + l] + deltax[l];
      const float ay = accumy[row + l] + deltay[l];
      const int kx = (int)ax, ky = (int)ay;
      k.kx[l] = kx; k.ky[l] = ky;
      fx[l] = ax - (float)kx; fy[l] = ay - (float)ky;
      if (e > e0 && (kx != g.k.kx[l] || ky != g.k.ky[l])) same = false;
    }
    if (!same) break;
    for (int l = 0; l < nl; l++) {
      if (e == e0) { g.k.kx[l] = k.kx[l]; g.k.ky[l] = k.ky[l]; g.fx[l] = fx[l]; g.fy[l] = fy[l]; }
      if (remx) { remx[row + l] = fx[l]; remy[row + l] = fy[l]; }
    }
  }
  g.n = e - e0;
  return g;
}

// does every one of n environments move by the same shift, and by which
static inline bool move_uniform(int nl, const float *accumx, const float *accumy, const float *deltax, const float *deltay,
                                int n, MoveShift &k) {
  const MoveGroup g = move_group(nl, accumx, accumy, nullptr, nullptr, deltax, deltay, 0, n);
  k = g.k;
  return g.n == n;
}

// ---- rounds
static inline int move_nrounds(const MoveShift &k, int nl) {
  int maxr = 0;
  for (int l = 0; l < nl; l++) {
    const int len = (k.kx[l] < 0 ? -k.kx[l] : k.kx[l]) + (k.ky[l] < 0 ? -k.ky[l] : k.ky[l]);
    if (len > maxr) maxr = len;
  }
  return maxr;
}
static inline RoundOps move_round(const MoveShift &k, int nl, int r) {
  RoundOps o;
  o.nops = 0;
  for (int l = 0; l < nl; l++) {
    const int ax = k.kx[l] < 0 ? -k.kx[l] : k.kx[l], ay = k.ky[l] < 0 ? -k.ky[l] : k.ky[l];
    if (r < ax) { o.layer[o.nops] = l; o.dir[o.nops] = k.kx[l] > 0 ? 1 : -1; o.tflag[o.nops] = 0; o.nops++; }
    else if (r < ax + ay) { o.layer[o.nops] = l; o.dir[o.nops] = k.ky[l] > 0 ? 2 : -2; o.tflag[o.nops] = 0; o.nops++; }
  }
  return o;
}
static inline int reset_nrounds(const AtmosFacts &f) {
  int maxr = 0;
  for (int l = 0; l < f.nlayers; l++) if (2 * f.dim[l] > maxr) maxr = 2 * f.dim[l];
  return maxr;
}
static inline RoundOps reset_round(const AtmosFacts &f, const float *deltax, bool transposed, int r) {
  RoundOps o;
  o.nops = 0;
  for (int l = 0; l < f.nlayers; l++)
    if (r < 2 * f.dim[l]) {
      const int dx = deltax[l] > 0.f ? 1 : -1;
      o.layer[o.nops] = l; o.dir[o.nops] = transposed ? 2 * dx : dx; o.tflag[o.nops] = transposed ? 1 : 0; o.nops++;
    }
  return o;
}

// the round behind `a` as k_extrude_sg wants it; false when `b` holds a layer that `a` does not (never the case for
// the rounds of a frame or of a reset: a layer's operations fill consecutive rounds from the first one on)
static inline bool next_round(const RoundOps &a, const RoundOps &b, RoundNext &nx) {
  nx.nops = b.nops;
  for (int i = 0; i < AOMARL_MAX_LAYERS; i++) { nx.idx[i] = -1; nx.dir[i] = 0; nx.tflag[i] = 0; }
  for (int j = 0; j < b.nops; j++) {
    int at = -1;
    for (int i = 0; i < a.nops; i++) if (a.layer[i] == b.layer[j]) at = i;
    if (at < 0) return false;
    nx.idx[at] = j; nx.dir[j] = b.dir[j]; nx.tflag[j] = b.tflag[j];
  }
  return b.nops > 0;
}

// ---- launches
enum LaunchKind { GATHER, PRODUCT, SCATTER, SCATTER_GATHER, MOVE_SMALL };
struct Launch {
  LaunchKind kind;
  RoundOps ops;          // the sub-round (all but MOVE_SMALL)
  RoundNext next;        // SCATTER_GATHER: the round whose gather it does
  MoveShift shift;       // MOVE_SMALL
  int ref, cls;          // the sub-round's class and a layer of it: dim, ns and [A|B] of the product
  int par;               // the Z / ZREF pair it reads or writes (SCATTER_GATHER: reads ZREF of par, gathers into the other)
  bool is_write;         // writes ring lines
  bool may_ride;
};
struct RoundCarry { bool gathered; int par; };      // from round to round of one range: is this round's Z there, in which pair
struct RoundLaunches {
  int n;
  Launch l[3 * AOMARL_MAX_LAYERS];
  RoundCarry carry;      // for the next round
};

// the launches of round `cur`; next: the round behind it, null behind the last one
static inline void round_launches(const RoundOps &cur, const RoundOps *next, const AtmosFacts &f, RoundCarry carry,
                                  RoundLaunches &out) {
  out.n = 0;
  for (int cls = 0; cls < f.nclass; cls++) {
    RoundOps ops;
    ops.nops = 0;
    int ref = -1;
    for (int i = 0; i < cur.nops; i++)
      if (f.abclass[cur.layer[i]] == cls) {
        ops.layer[ops.nops] = cur.layer[i]; ops.dir[ops.nops] = cur.dir[i];
        ops.tflag[ops.nops] = cur.tflag[i]; ops.nops++; ref = cur.layer[i];
      }
    if (ops.nops == 0) continue;
    const bool single = ops.nops == cur.nops;
    RoundNext nx;
    // (k_extrude_sg keeps a column's whole index list in registers: SG_U entries per thread)
    bool fuse_next = single && !f.unfused && f.ns[ref] <= SG_U * SG_THREADS && f.dim[ref] <= SG_MAX_N && next &&
                     next_round(cur, *next, nx);
    if (fuse_next)                               // (the next round must be one sub-round too: same class)
      for (int i = 0; i < next->nops; i++) fuse_next = fuse_next && f.abclass[next->layer[i]] == cls;
    auto add = [&](LaunchKind kind) -> Launch & {
      Launch &a = out.l[out.n++];
      a.kind = kind; a.ops = ops; a.ref = ref; a.cls = cls; a.par = carry.par; a.is_write = false; a.may_ride = false;
      return a;
    };
    if (!(carry.gathered && single)) add(GATHER);
    add(PRODUCT);
    Launch &s = add(fuse_next ? SCATTER_GATHER : SCATTER);
    s.is_write = true;
    if (fuse_next) {
      s.next = nx;
      carry.par ^= 1; carry.gathered = true;
    } else {
      s.may_ride = !next && cls + 1 == f.nclass;
      carry.gathered = false;
    }
  }
  out.carry = carry;
}

// ---- a group's move
struct GroupPlan {
  int nrounds;           // 0: the group does not move, nothing is launched
  bool small;            // the one launch small_launch() instead of the rounds
  bool overlap;          // may run beside the older frame in flight (false when there is none)
  bool complete;
};
static inline GroupPlan group_plan(const MoveShift &k, const AtmosFacts &f, bool older_in_flight) {
  GroupPlan p;
  p.nrounds = move_nrounds(k, f.nlayers);
  p.small = p.nrounds > 0 && f.small;
  p.complete = true;
  for (int l = 0; l < f.nlayers; l++)
    if (k.kx[l] == 0 && k.ky[l] == 0) p.complete = false;
  // The extrusions rewrite the |kx| oldest columns / |ky| oldest rows of each ring (logical 0.. for a positive shift,
  // dim-1.. for a negative one): outside every window the one-pass frame kernel reads  <=>  within the margins around
  // the pupil
  p.overlap = older_in_flight && p.nrounds > 0;
  if (p.overlap)
    for (int l = 0; l < f.nlayers; l++) {
      const int lox = f.tox[l], hix = f.dim[l] - f.tox[l] - f.pupdiam, loy = f.toy[l], hiy = f.dim[l] - f.toy[l] - f.pupdiam;
      if ((k.kx[l] > 0 ? k.kx[l] > lox : -k.kx[l] > hix) || (k.ky[l] > 0 ? k.ky[l] > loy : -k.ky[l] > hiy)) p.overlap = false;
    }
  return p;
}
static inline Launch small_launch(const MoveShift &k) {
  Launch s;
  s.kind = MOVE_SMALL; s.shift = k; s.ops.nops = 0; s.ref = -1; s.cls = -1; s.par = 0;
  s.is_write = true;                             // it reads AND writes the rings
  s.may_ride = true;                             // the group's whole move in this one launch
  return s;
}

// ---- reset partition
struct ResetFacts {
  int reset_streams;     // "reset_streams"
  bool prefetch_atmos, capturing;
  bool whole;            // the prefetched reset with "reset_prefetch_whole" (the plain reset: false)
};
// In how many parts a reset of n environments walks its rounds (each part's products have its own columns: the
// partition fixes the split-K order of every sum, so the prefetched reset uses the plain one's)
static inline int reset_parts(const ResetFacts &f, int n) {
  if (f.reset_streams > 1 && f.prefetch_atmos && n >= 16 * f.reset_streams && !f.capturing)
    return f.reset_streams > 4 ? 4 : f.reset_streams;
  return 1;
}
struct ResetPart { int b, n, pick_n; };   // pick_n > 0: the products take the tile and k split a range of pick_n environments would get
static inline int reset_partition(const ResetFacts &f, int b, int n, ResetPart out[4]) {
  const int parts = reset_parts(f, n);
  if (f.whole && parts > 1 && n % parts == 0) {
    out[0] = ResetPart{b, n, n / parts};
    return 1;
  }
  int e0 = b;
  for (int k = 0; k < parts; k++) {
    const int nk = (b + n - e0) / (parts - k);
    out[k] = ResetPart{e0, nk, 0};
    e0 += nk;
  }
  return parts;
}
