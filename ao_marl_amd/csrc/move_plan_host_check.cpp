// move_plan_host_check.cpp -- a stand-alone host program around aomarl_move_plan_host.h (the launch sequence of a move
// or a reset of the atmosphere), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o move_plan_host_check move_plan_host_check.cpp
// No GPU, no HIP.  It walks the plan the way the executor in aomarl_capi_atmos.hip does -- group by group, round by
// round, run by run -- over every combination of 1..3 layers, one and two [A|B] classes, shifts in {-2..2}^2 per layer,
// "extrude_unfused" on and off and the line lengths k_extrude_sg takes just inside and just outside, and requires what
// the header's comment promises; then groups, verdicts and the reset partition.  Exit status 0: all held, and the line
// "move_plan_host_check: ok (<count> combinations)".
//     move_plan_host_check --table     also prints the launch sequence of a fixed list of cases, one line per launch
//                                      record (tests/test_move_plan.py compares it with tests/golden/move_plans.txt)
#include "aomarl_move_plan_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); exit(1); } \
  } while (0)

static const int NL_MAX = 3;
static const char *const kKind[] = {"GATHER", "PRODUCT", "SCATTER", "SCATTER_GATHER", "MOVE_SMALL"};

static AtmosFacts facts(int nl, const int *abclass, const int *dim, const int *ns, bool unfused, bool small) {
  AtmosFacts f;
  memset(&f, 0, sizeof(f));
  f.nlayers = nl; f.nclass = 0;
  for (int l = 0; l < nl; l++) {
    f.abclass[l] = abclass[l]; f.dim[l] = dim[l]; f.ns[l] = ns[l]; f.tox[l] = 1; f.toy[l] = 2;
    if (abclass[l] + 1 > f.nclass) f.nclass = abclass[l] + 1;
  }
  f.pupdiam = 2; f.unfused = unfused; f.small = small;
  return f;
}

// ---- the table's lines
static void print_launch(const char *who, int r, const Launch &L) {
  printf("%s r%d %s ref %d par %d w %d ride %d", who, r, kKind[L.kind], L.ref, L.par, L.is_write ? 1 : 0, L.may_ride ? 1 : 0);
  if (L.kind == MOVE_SMALL) {
    printf(" shift");
    for (int l = 0; l < AOMARL_MAX_LAYERS; l++) printf(" %d:%d", L.shift.kx[l], L.shift.ky[l]);
  } else {
    printf(" ops");
    for (int i = 0; i < L.ops.nops; i++) printf(" %d:%d:%d", L.ops.layer[i], L.ops.dir[i], L.ops.tflag[i]);
  }
  if (L.kind == SCATTER_GATHER) {
    printf(" next %d idx", L.next.nops);
    for (int i = 0; i < AOMARL_MAX_LAYERS; i++) printf(" %d", L.next.idx[i]);
    printf(" dir");
    for (int i = 0; i < AOMARL_MAX_LAYERS; i++) printf(" %d", L.next.dir[i]);
    printf(" t");
    for (int i = 0; i < AOMARL_MAX_LAYERS; i++) printf(" %d", L.next.tflag[i]);
  }
  printf("\n");
}
static void print_group(const MoveGroup &g, int nl, const GroupPlan &p) {
  printf("group %d %d shift", g.b, g.n);
  for (int l = 0; l < nl; l++) printf(" %d:%d", g.k.kx[l], g.k.ky[l]);
  printf(" rounds %d small %d overlap %d complete %d\n", p.nrounds, p.small ? 1 : 0, p.overlap ? 1 : 0, p.complete ? 1 : 0);
}
static void print_floats(const char *what, const float *v, size_t n) {
  printf("%s", what);
  for (size_t i = 0; i < n; i++) printf(" %a", (double)v[i]);
  printf("\n");
}

// ---- the executor's walk, launches collected instead of launched
struct Rec { int r; Launch l; };
struct Run {               // ExtrudeRun without a GPU
  RoundCarry carry = {false, 0};
  std::vector<Rec> recs;
  void round(const RoundOps &cur, const RoundOps *next, const AtmosFacts &f, int r) {
    RoundLaunches rl;
    round_launches(cur, next, f, carry, rl);
    REQUIRE(rl.n >= 0 && rl.n <= 3 * f.nclass);
    for (int i = 0; i < rl.n; i++) recs.push_back(Rec{r, rl.l[i]});
    carry = rl.carry;
  }
};
static std::vector<Rec> walk_group(const MoveShift &k, const AtmosFacts &f, const GroupPlan &gp) {
  Run run;
  if (gp.nrounds == 0) return run.recs;
  if (gp.small) { run.recs.push_back(Rec{0, small_launch(k)}); return run.recs; }
  for (int r = 0; r < gp.nrounds; r++) {
    const RoundOps cur = move_round(k, f.nlayers, r), next = move_round(k, f.nlayers, r + 1);
    run.round(cur, r + 1 < gp.nrounds ? &next : nullptr, f, r);
  }
  return run.recs;
}

// ---- what must hold of one group's records
static void check_group(const MoveShift &k, const AtmosFacts &f, const std::vector<Rec> &recs) {
  const int nl = f.nlayers, nrounds = move_nrounds(k, nl);
  int nx[NL_MAX] = {0, 0, 0}, ny[NL_MAX] = {0, 0, 0};
  int par = 0, rides = 0;
  bool have_gather = false, have_product = false, first_write_seen = false;
  int gather_par = 0;
  for (size_t i = 0; i < recs.size(); i++) {
    const Launch &L = recs[i].l;
    const int r = recs[i].r;
    const RoundOps cur = move_round(k, nl, r), next = move_round(k, nl, r + 1);
    REQUIRE(L.ops.nops > 0 && L.ref >= 0 && f.abclass[L.ref] == L.cls);
    for (int j = 0; j < L.ops.nops; j++) REQUIRE(f.abclass[L.ops.layer[j]] == L.cls);
    REQUIRE(L.par == par);
    REQUIRE(L.is_write == (L.kind == SCATTER || L.kind == SCATTER_GATHER));
    if (L.is_write) first_write_seen = true;
    if (L.kind == GATHER) {
      REQUIRE(!have_gather && !have_product);
      have_gather = true; gather_par = L.par;
    } else if (L.kind == PRODUCT) {
      REQUIRE(have_gather && !have_product && L.par == gather_par);       // it reads what its gather wrote
      have_product = true;
    } else {
      REQUIRE(L.kind == SCATTER || L.kind == SCATTER_GATHER);
      REQUIRE(have_gather && have_product);
      have_gather = have_product = false;
      for (int j = 0; j < L.ops.nops; j++) {                               // x lines first, then y lines, with the shift's signs
        const int l = L.ops.layer[j], d = L.ops.dir[j];
        REQUIRE(L.ops.tflag[j] == 0);
        if (d == 1 || d == -1) { REQUIRE(ny[l] == 0 && d == (k.kx[l] > 0 ? 1 : -1)); nx[l]++; }
        else { REQUIRE((d == 2 || d == -2) && nx[l] == abs(k.kx[l]) && d == (k.ky[l] > 0 ? 2 : -2)); ny[l]++; }
      }
      bool same_class = next.nops > 0;
      for (int j = 0; j < next.nops; j++) same_class = same_class && f.abclass[next.layer[j]] == L.cls;
      RoundNext want;
      const bool fuses = L.ops.nops == cur.nops && r + 1 < nrounds && same_class && next_round(cur, next, want) &&
                         f.ns[L.ref] <= SG_U * SG_THREADS && f.dim[L.ref] <= SG_MAX_N && !f.unfused;
      REQUIRE((L.kind == SCATTER_GATHER) == fuses);
      if (L.kind == SCATTER_GATHER) {
        REQUIRE(!memcmp(&want, &L.next, sizeof(want)) && !L.may_ride);
        par ^= 1;                                                          // the parity flips here and nowhere else
        have_gather = true; gather_par = par;                              // the next round's gather is done
      }
    }
    if (L.may_ride) { rides++; REQUIRE(i + 1 == recs.size() && L.kind == SCATTER && r + 1 == nrounds && L.cls + 1 == f.nclass); }
  }
  REQUIRE(!have_gather && !have_product && rides <= 1);
  REQUIRE(first_write_seen == (nrounds > 0));
  for (int l = 0; l < nl; l++) REQUIRE(nx[l] == abs(k.kx[l]) && ny[l] == abs(k.ky[l]));
  // something rides exactly when the last class index has an operation in the last round
  if (nrounds > 0) {
    const RoundOps last = move_round(k, nl, nrounds - 1);
    bool has = false;
    for (int j = 0; j < last.nops; j++) has = has || f.abclass[last.layer[j]] == f.nclass - 1;
    REQUIRE((rides == 1) == has);
  }
}

static unsigned long long check_rounds() {
  unsigned long long count = 0, fused = 0, thinned = 0;
  // class assignments: one class, and every way of using exactly two (layer 0 in class 0)
  const int assign[NL_MAX + 1][4][NL_MAX] = {{}, {{0}}, {{0, 0}, {0, 1}}, {{0, 0, 0}, {0, 0, 1}, {0, 1, 0}, {0, 1, 1}}};
  const int nassign[NL_MAX + 1] = {0, 1, 2, 4};
  const int lim[3][2] = {{SG_MAX_N, SG_U * SG_THREADS}, {SG_MAX_N + 1, SG_U * SG_THREADS}, {SG_MAX_N, SG_U * SG_THREADS + 1}};
  for (int nl = 1; nl <= NL_MAX; nl++)
    for (int a = 0; a < nassign[nl]; a++)
      for (int v = 0; v < 3; v++)
        for (int unfused = 0; unfused < 2; unfused++) {
          const int dim[NL_MAX] = {lim[v][0], lim[v][0], lim[v][0]}, ns[NL_MAX] = {lim[v][1], lim[v][1], lim[v][1]};
          const AtmosFacts f = facts(nl, assign[nl][a], dim, ns, unfused != 0, false);
          int total = 1;
          for (int l = 0; l < nl; l++) total *= 25;
          for (int code = 0; code < total; code++) {
            MoveShift k;
            memset(&k, 0, sizeof(k));
            for (int l = 0, c = code; l < nl; l++, c /= 25) { k.kx[l] = c % 5 - 2; k.ky[l] = (c % 25) / 5 - 2; }
            const GroupPlan gp = group_plan(k, f, false);
            const std::vector<Rec> recs = walk_group(k, f, gp);
            check_group(k, f, recs);
            bool moves_all = true, moves_any = false;
            for (int l = 0; l < nl; l++) {
              const bool m = k.kx[l] != 0 || k.ky[l] != 0;
              moves_all = moves_all && m; moves_any = moves_any || m;
            }
            REQUIRE(gp.complete == moves_all && (gp.nrounds > 0) == moves_any && !gp.small && !gp.overlap);
            for (const Rec &rc : recs) {
              if (rc.l.kind == SCATTER_GATHER) { fused++; if (rc.l.next.nops < rc.l.ops.nops) thinned++; }
              REQUIRE(!(v || unfused) || rc.l.kind != SCATTER_GATHER);
            }
            // the small move: one record that writes and may ride
            AtmosFacts fs = f;
            fs.small = true;
            const GroupPlan gs = group_plan(k, fs, false);
            const std::vector<Rec> one = walk_group(k, fs, gs);
            REQUIRE(gs.small == moves_any && one.size() == (moves_any ? 1u : 0u));
            if (moves_any) REQUIRE(one[0].l.kind == MOVE_SMALL && one[0].l.is_write && one[0].l.may_ride && !memcmp(&one[0].l.shift, &k, sizeof(k)));
            count++;
          }
        }
  REQUIRE(fused > 0 && thinned > 0);
  return count;
}

// ---- overlap: the margin predicate, over shifts and margins
static unsigned long long check_overlap() {
  unsigned long long count = 0;
  const int abc[NL_MAX] = {0, 0, 0}, ns[NL_MAX] = {8, 8, 8};
  for (int tox = 0; tox <= 3; tox++)
    for (int toy = 0; toy <= 3; toy++)
      for (int dim = 4; dim <= 8; dim++)
        for (int kx = -2; kx <= 2; kx++)
          for (int ky = -2; ky <= 2; ky++)
            for (int k2 = -2; k2 <= 2; k2++) {
              const int dims[NL_MAX] = {dim, 8, 8};
              AtmosFacts f = facts(2, abc, dims, ns, false, false);
              f.tox[0] = tox; f.toy[0] = toy; f.tox[1] = 2; f.toy[1] = 2; f.pupdiam = 3;
              MoveShift k;
              memset(&k, 0, sizeof(k));
              k.kx[0] = kx; k.ky[0] = ky; k.kx[1] = k2;
              auto fits = [&](int s, int lo, int hi) { return s > 0 ? s <= lo : -s <= hi; };
              const bool want = fits(kx, tox, dim - tox - 3) && fits(ky, toy, dim - toy - 3) && fits(k2, 2, 3);
              const bool moves = kx || ky || k2;
              REQUIRE(group_plan(k, f, true).overlap == (want && moves));
              REQUIRE(!group_plan(k, f, false).overlap);
              count++;
            }
  return count;
}

// ---- groups: a partition in order, members share a shift, neighbours differ; uniform <=> one group
static std::vector<MoveGroup> groups_of(int nl, std::vector<float> &ax, std::vector<float> &ay, const float *dx, const float *dy, int b, int n) {
  std::vector<MoveGroup> gs;
  for (int e = b; e < b + n;) {
    gs.push_back(move_group(nl, ax.data(), ay.data(), ax.data(), ay.data(), dx, dy, e, b + n));
    REQUIRE(gs.back().b == e && gs.back().n >= 1);
    e += gs.back().n;
  }
  return gs;
}
static unsigned long long check_groups() {
  unsigned long long count = 0;
  const float dx[2] = {0.625f, -0.375f}, dy[2] = {0.25f, 1.5f};
  const float start[4] = {0.f, 0.5f, -0.75f, 1.875f};
  const int n = 5, nl = 2;
  for (int code = 0; code < 1024; code++) {                   // every environment one of 4 starting values, layer 1 offset
    std::vector<float> ax((size_t)n * nl), ay((size_t)n * nl);
    for (int e = 0, c = code; e < n; e++, c /= 4) {
      ax[e * nl] = start[c % 4]; ax[e * nl + 1] = -start[c % 4]; ay[e * nl] = start[(c + 1) % 4]; ay[e * nl + 1] = 0.125f;
    }
    const std::vector<float> ax0 = ax, ay0 = ay;
    MoveShift ku;
    const bool uniform = move_uniform(nl, ax.data(), ay.data(), dx, dy, n, ku);
    REQUIRE(ax == ax0 && ay == ay0);                           // a question writes nothing
    const std::vector<MoveGroup> gs = groups_of(nl, ax, ay, dx, dy, 0, n);
    REQUIRE(uniform == (gs.size() == 1));
    REQUIRE(!memcmp(&ku, &gs[0].k, sizeof(ku)));
    int e = 0;
    for (size_t g = 0; g < gs.size(); g++) {
      REQUIRE(gs[g].b == e);
      for (int m = e; m < e + gs[g].n; m++)
        for (int l = 0; l < nl; l++) {
          const float sx = ax0[m * nl + l] + dx[l], sy = ay0[m * nl + l] + dy[l];
          REQUIRE(gs[g].k.kx[l] == (int)sx && gs[g].k.ky[l] == (int)sy);
          REQUIRE(ax[m * nl + l] == sx - (float)(int)sx && ay[m * nl + l] == sy - (float)(int)sy);
          if (m == e) REQUIRE(gs[g].fx[l] == ax[m * nl + l] && gs[g].fy[l] == ay[m * nl + l]);
        }
      if (g) REQUIRE(memcmp(&gs[g].k, &gs[g - 1].k, sizeof(MoveShift)) != 0);
      e += gs[g].n;
    }
    REQUIRE(e == n);
    count++;
  }
  return count;
}

// ---- the reset partition
static unsigned long long check_reset() {
  unsigned long long count = 0;
  const int ns[9] = {15, 16, 31, 32, 33, 64, 65, 255, 256};
  for (int n : ns)
    for (int streams = 1; streams <= 4; streams++)
      for (int bits = 0; bits < 8; bits++)
        for (int b = 0; b <= 3; b += 3) {
          const ResetFacts f = {streams, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0};
          const int parts = reset_parts(f, n);
          REQUIRE(parts == ((streams > 1 && n >= 16 * streams && f.prefetch_atmos && !f.capturing) ? streams : 1));
          ResetPart p[4];
          const int np = reset_partition(f, b, n, p);
          if (f.whole && parts > 1 && n % parts == 0) {
            REQUIRE(np == 1 && p[0].b == b && p[0].n == n && p[0].pick_n == n / parts);
          } else {
            REQUIRE(np == parts);
            int e0 = b;
            for (int k = 0; k < np; k++) {
              REQUIRE(p[k].b == e0 && p[k].n == (b + n - e0) / (parts - k) && p[k].pick_n == 0 && p[k].n > 0);
              e0 += p[k].n;
            }
            REQUIRE(e0 == b + n);
          }
          count++;
        }
  { const ResetFacts f = {7, true, false, false}; REQUIRE(reset_parts(f, 112) == 4 && reset_parts(f, 111) == 1); }
  return count;
}

// ---- the table
static float accum_for(int k) { return k >= 0 ? (float)k - 0.25f : (float)k - 0.75f; }      // with delta 0.5: shift k, remainder +-0.25
struct MoveCase {
  const char *name;
  int nl, abclass[NL_MAX], dim[NL_MAX], ns[NL_MAX];
  bool unfused, small, older;
  int nenv;
  int kx[6][NL_MAX], ky[6][NL_MAX];      // per environment
};
static const MoveCase kMoves[] = {
    // three layers of one class that finish at rounds 1, 3 and 2: the rounds thin out (RoundNext), y lines behind x lines
    {"thin3", 3, {0, 0, 0}, {8, 8, 8}, {6, 6, 6}, false, false, false, 1, {{1, 2, -1}}, {{0, 1, -1}}},
    {"thin3_unfused", 3, {0, 0, 0}, {8, 8, 8}, {6, 6, 6}, true, false, false, 1, {{1, 2, -1}}, {{0, 1, -1}}},
    {"thin3_small", 3, {0, 0, 0}, {8, 8, 8}, {6, 6, 6}, false, true, false, 1, {{1, 2, -1}}, {{0, 1, -1}}},
    {"thin3_long_stencil", 3, {0, 0, 0}, {8, 8, 8}, {SG_U * SG_THREADS + 1, SG_U * SG_THREADS + 1, SG_U * SG_THREADS + 1}, false, false, false, 1, {{1, 2, -1}}, {{0, 1, -1}}},
    {"thin3_long_line", 3, {0, 0, 0}, {SG_MAX_N + 1, SG_MAX_N + 1, SG_MAX_N + 1}, {6, 6, 6}, false, false, false, 1, {{1, 2, -1}}, {{0, 1, -1}}},
    // two classes: nothing fuses while both have work; the last round is class 0 alone, nothing may ride
    {"two_class", 3, {0, 1, 0}, {8, 6, 8}, {6, 5, 6}, false, false, false, 1, {{1, 1, 2}}, {{0, 0, 1}}},
    {"two_class_last_rides", 2, {0, 1}, {8, 6}, {6, 5}, false, false, false, 1, {{1, 2}}, {{0, 0}}},
    {"y_behind_x", 1, {0}, {8}, {6}, false, false, false, 1, {{1}}, {{-2}}},
    // six environments in three groups: [0, 2) moves, [2, 3) does not, [3, 6) takes a two-pixel step in layer 1
    {"three_groups", 3, {0, 0, 0}, {8, 8, 8}, {6, 6, 6}, false, false, false, 6,
     {{1, 0, 0}, {1, 0, 0}, {0, 0, 0}, {0, 2, 1}, {0, 2, 1}, {0, 2, 1}}, {{0, 1, 0}, {0, 1, 0}, {0, 0, 0}, {0, 0, -1}, {0, 0, -1}, {0, 0, -1}}},
    {"three_groups_small", 3, {0, 0, 0}, {8, 8, 8}, {6, 6, 6}, false, true, false, 6,
     {{1, 0, 0}, {1, 0, 0}, {0, 0, 0}, {0, 2, 1}, {0, 2, 1}, {0, 2, 1}}, {{0, 1, 0}, {0, 1, 0}, {0, 0, 0}, {0, 0, -1}, {0, 0, -1}, {0, 0, -1}}},
    // an older frame in flight (margins: tox 1, toy 2, dim - to - pupdiam = 5 / 4): inside, then one pixel too far
    {"older_inside", 2, {0, 0}, {8, 8}, {6, 6}, false, false, true, 1, {{1, -2}}, {{2, 0}}},
    {"older_outside", 2, {0, 0}, {8, 8}, {6, 6}, false, false, true, 1, {{2, 0}}, {{0, 0}}},
    {"older_two_groups", 2, {0, 0}, {8, 8}, {6, 6}, false, false, true, 2, {{1, 1}, {2, 1}}, {{0, 0}, {0, 0}}},
};

static void table_move(const MoveCase &m) {
  const AtmosFacts f = facts(m.nl, m.abclass, m.dim, m.ns, m.unfused, m.small);
  float dx[NL_MAX], dy[NL_MAX];
  std::vector<float> ax((size_t)m.nenv * m.nl), ay((size_t)m.nenv * m.nl);
  for (int l = 0; l < m.nl; l++) { dx[l] = 0.5f; dy[l] = 0.5f; }
  for (int e = 0; e < m.nenv; e++)
    for (int l = 0; l < m.nl; l++) { ax[e * m.nl + l] = accum_for(m.kx[e][l]); ay[e * m.nl + l] = accum_for(m.ky[e][l]); }
  printf("# move %s: layers %d unfused %d small %d older %d environments %d\n", m.name, m.nl, m.unfused, m.small, m.older, m.nenv);
  MoveShift ku;
  printf("uniform %d\n", move_uniform(m.nl, ax.data(), ay.data(), dx, dy, m.nenv, ku) ? 1 : 0);
  bool complete = true;
  for (int e = 0; e < m.nenv;) {
    const MoveGroup g = move_group(m.nl, ax.data(), ay.data(), ax.data(), ay.data(), dx, dy, e, m.nenv);
    if (e == 0) { print_floats("frac_x", g.fx, m.nl); print_floats("frac_y", g.fy, m.nl); }
    e += g.n;
    const GroupPlan gp = group_plan(g.k, f, m.older);
    complete = complete && gp.complete;
    print_group(g, m.nl, gp);
    for (const Rec &rc : walk_group(g.k, f, gp)) print_launch("  ", rc.r, rc.l);
  }
  printf("complete %d\n", complete ? 1 : 0);
  print_floats("accum_x", ax.data(), ax.size());
  print_floats("accum_y", ay.data(), ay.size());
}

struct ResetCase {
  const char *name;
  bool transposed, unfused;
  float deltax[2];
  int b, n, streams;
  bool prefetch_atmos, capturing, prefetched, whole;
  int advance;           // the prefetched reset: rounds per call
};
static const ResetCase kResets[] = {
    {"transposed", true, false, {0.5f, -0.5f}, 0, 4, 2, true, false, false, false, 0},
    {"untransposed", false, false, {0.5f, -0.5f}, 0, 4, 2, true, false, false, false, 0},
    {"two_parts", true, false, {0.5f, 0.5f}, 3, 33, 2, true, false, false, false, 0},
    {"capturing_one_part", true, false, {0.5f, 0.5f}, 0, 32, 2, true, true, false, false, 0},
    {"prefetched_whole_by_two", true, false, {0.5f, 0.5f}, 0, 32, 2, true, false, true, true, 2},
    {"prefetched_parts_by_two", true, false, {0.5f, 0.5f}, 0, 33, 2, true, false, true, true, 2},
    {"prefetched_unfused_by_five", true, true, {-0.5f, 0.5f}, 0, 64, 4, true, false, true, false, 5},
};
// two small layers of different size: dims 4 and 6, a class each
static void table_reset(const ResetCase &t) {
  const int abclass[2] = {0, 1}, dim[2] = {4, 6}, ns[2] = {5, 7};
  const AtmosFacts f = facts(2, abclass, dim, ns, t.unfused, false);
  const ResetFacts rf = {t.streams, t.prefetch_atmos, t.capturing, t.prefetched && t.whole};
  printf("# reset %s: transposed %d unfused %d environments [%d, %d) streams %d prefetch_atmos %d capturing %d prefetched %d whole %d\n",
         t.name, t.transposed, t.unfused, t.b, t.b + t.n, t.streams, t.prefetch_atmos, t.capturing, t.prefetched, t.whole);
  const int nrounds = reset_nrounds(f);
  std::vector<RoundOps> rounds;
  for (int r = 0; r < nrounds; r++) rounds.push_back(reset_round(f, t.deltax, t.transposed, r));
  ResetPart part[4];
  const int parts = reset_partition(rf, t.b, t.n, part);
  printf("rounds %d parts %d:", nrounds, parts);
  for (int k = 0; k < parts; k++) printf(" %d %d pick %d", part[k].b, part[k].n, part[k].pick_n);
  printf("\n");
  std::vector<Run> runs((size_t)parts);
  for (int r = 0; r < nrounds; r++) {
    if (t.prefetched && r % t.advance == 0) printf("advance %d\n", t.advance);
    for (int k = 0; k < parts; k++) {
      runs[k].recs.clear();
      runs[k].round(rounds[r], r + 1 < nrounds ? &rounds[r + 1] : nullptr, f, r);
      char who[16];
      snprintf(who, sizeof(who), "  p%d", k);
      for (const Rec &rc : runs[k].recs) {
        REQUIRE(!rc.l.may_ride || (r + 1 == nrounds && rc.l.kind == SCATTER));
        print_launch(who, rc.r, rc.l);
      }
    }
  }
}

int main(int argc, char **argv) {
  const bool table = argc >= 2 && !strcmp(argv[1], "--table");
  unsigned long long count = check_rounds();
  count += check_overlap();
  count += check_groups();
  count += check_reset();
  if (table) {
    for (const MoveCase &m : kMoves) table_move(m);
    for (const ResetCase &t : kResets) table_reset(t);
  }
  printf("move_plan_host_check: ok (%llu combinations)\n", count);
  return 0;
}
