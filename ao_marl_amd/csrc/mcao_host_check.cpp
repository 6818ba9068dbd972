// mcao_host_check.cpp -- a stand-alone host program around the host half of multi-conjugate AO (aomarl_mcao_host.h: the
// validation of the desc, of the views and of the calls, the shape launch's plan, the add kernel's offset table) and the
// field's offset table for attached mirrors (aomarl_field_host.h), meant to be built with the address and
// undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o mcao_host_check mcao_host_check.cpp
// No GPU, no HIP.  Exit status 0: all held.
#include "aomarl_mcao_host.h"
#include "aomarl_field_host.h"

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main() {
  std::string err;
  // ---- the desc: two mirrors, pitch 8, a profile of 34 pixels
  const int gw0 = 19, gw1 = 30, ss = 34, pitch = 8;
  std::vector<int32_t> g0(gw0 * gw0, -1), g1(gw1 * gw1, -1);
  int n0 = 0, n1 = 0;
  for (int i = 0; i < gw0 * gw0; i++) if (i % 7) g0[i] = n0++;
  for (int i = 0; i < gw1 * gw1; i++) if (i % 5) g1[i] = n1++;
  std::vector<float> prof(ss, 0.05f);
  aomarl_mcao_desc ok = {};
  ok.nmirrors = 2;
  ok.mirrors[0] = {4500.f, 180, pitch, 0, 0, gw0, gw0, ss, n0, g0.data(), prof.data()};
  ok.mirrors[1] = {14000.f, 268, pitch, 1, 1, gw1, gw1, ss, n1, g1.data(), prof.data()};
  void *outp = &err;
  REQUIRE(mcao_validate_desc(&ok, 3, outp, err) == 0);
  REQUIRE(mcao_validate_desc(nullptr, 3, outp, err) == 1 && has(err, "null desc"));
  REQUIRE(mcao_validate_desc(&ok, 3, nullptr, err) == 1 && has(err, "null output pointer"));
  for (int v : {0, 3, -1}) { auto d = ok; d.nmirrors = v; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "mirrors: 1..2")); }
  REQUIRE(mcao_validate_desc(&ok, 0, outp, err) == 1 && has(err, "environments: at least one"));
  for (float v : {-1.f, NAN, INFINITY}) { auto d = ok; d.mirrors[1].alt = v; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "mirror 1: alt")); }
  { auto d = ok; d.mirrors[0].grid = nullptr; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "mirror 0: null grid / prof")); }
  { auto d = ok; d.mirrors[1].prof = nullptr; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "mirror 1: null grid / prof")); }
  { auto d = ok; d.mirrors[0].pitch = 0; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "sizes must be positive")); }
  { auto d = ok; d.mirrors[0].nact = gw0 * gw0 + 1; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "sizes must be positive")); }
  // a lattice that leaves the plane: the last patch ends at 1 + 8 * 29 + 34 = 267 <= 268; one pixel further it does not
  { auto d = ok; d.mirrors[1].i1min = 3; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "mirror 1: the lattice leaves the plane")); }
  { auto d = ok; d.mirrors[1].i1min = 2; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 0); }
  { auto d = ok; d.mirrors[0].j1min = -1; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "mirror 0: the lattice leaves the plane")); }
  { auto d = ok; d.mirrors[0].dim = 177; REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "the lattice leaves the plane")); }
  for (int v : {-2, n0}) { auto g = g0; g[11] = v; auto d = ok; d.mirrors[0].grid = g.data(); REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "grid entry 11")); }
  { auto g = g0; g[11] = n0 - 1; auto d = ok; d.mirrors[0].grid = g.data(); REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 0); }
  // the profile against the shape kernel's LDS patch: 12 cells per axis, 128 pixels
  { std::vector<float> p(129, 0.f); auto d = ok; d.mirrors[0].ss = 129; d.mirrors[0].pitch = 64; d.mirrors[0].gw = d.mirrors[0].gh = 1; d.mirrors[0].nact = 1; d.mirrors[0].prof = p.data();
    REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "larger than the shape kernel's LDS patch")); }
  { auto d = ok; d.mirrors[0].pitch = 5; d.mirrors[0].gw = d.mirrors[0].gh = 4; d.mirrors[0].nact = 12;      // (32 + 32) / 5 + 2 = 14 cells > 12
    REQUIRE(mcao_cells_needed(ss, 5) == 14);
    REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "larger than the shape kernel's LDS patch")); }
  REQUIRE(mcao_cells_needed(ss, pitch) == 10 && mcao_cells_needed(56, 16) == 7);
  { auto p = prof; p[3] = NAN; auto d = ok; d.mirrors[1].prof = p.data(); REQUIRE(mcao_validate_desc(&d, 3, outp, err) == 1 && has(err, "prof[3] is not finite")); }
  REQUIRE(mcao_validate_desc(&ok, 20000, outp, err) == 1 && has(err, "2^31"));
  // every cell the kernel can reach from a tile lies in its patch: walk the tiles of mirror 1 as the kernel does
  {
    const aomarl_mcao_mirror &M = ok.mirrors[1];
    for (int x0 = 0; x0 < M.dim; x0 += MCAO_TILE) {
      const int num = x0 - M.i1min - (M.ss - 1);
      const int gb = num >= 0 ? (num + M.pitch - 1) / M.pitch : -((-num) / M.pitch);
      for (int g = 0; g < M.gw; g++) {
        const int X = M.i1min + M.pitch * g;
        const bool touches = X + M.ss - 1 >= x0 && X <= x0 + MCAO_TILE - 1;
        if (touches) REQUIRE(g >= gb && g < gb + MCAO_CELLS);
      }
    }
  }

  // ---- the ranges
  REQUIRE(mcao_validate_range("mcao_apply", 4, 0, 4, err) == 0);
  REQUIRE(mcao_validate_range("mcao_apply", 4, 2, 3, err) == 1 && has(err, "mcao_apply: environments 2 .. +3 of 4"));
  REQUIRE(mcao_validate_range("mcao_reset", 4, -1, 2, err) == 1 && has(err, "mcao_reset: environments"));
  REQUIRE(mcao_validate_range("mcao_reset", 4, 0, 0, err) == 1 && has(err, "environments"));

  // ---- the view and the add: 3 directions on a sensor grid of 84 and a pupil grid of 80
  const int n = 84, pd = 80, dims[2] = {180, 268};
  std::vector<float> off = {48.f, 48.f, 92.f, 92.f, 65.45f, 48.f, 146.3f, 92.f, 39.3f, 61.1f, 64.9f, 132.7f};
  std::vector<float> dm1 = {0.f, 0.f, -0.05f, -0.1556f, -0.075f, -0.2333f};
  float planes[1];
  aomarl_mcao_view v = {3, off.data(), dm1.data()};
  const int known = AOMARL_TRACE_MASK;
  REQUIRE(mcao_validate_add(&v, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 0);
  REQUIRE(mcao_validate_add(&v, planes, 3, n, n, pd, 2, dims, 4, 1, 3, known, known, err) == 0);
  REQUIRE(mcao_validate_add(&v, nullptr, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "null planes"));
  REQUIRE(mcao_validate_add(nullptr, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "null view"));
  for (int k : {0, 9, -1}) REQUIRE(mcao_validate_add(&v, planes, k, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "directions: 1..8"));
  { auto w = v; w.ndir = 9; REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "9 directions: 1..8")); }
  { auto w = v; w.ndir = 2; REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "the view has 2 directions, the planes 3")); }
  REQUIRE(mcao_validate_add(&v, planes, 3, 82, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "a grid of 82 pixels"));
  { auto w = v; w.off = nullptr; REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "null off / dm1")); }
  { auto w = v; w.dm1 = nullptr; REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "null off / dm1")); }
  for (float x : {NAN, INFINITY}) { auto o = off; o[5] = x; auto w = v; w.off = o.data(); REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "off of direction 1, mirror 0 is not finite")); }
  for (float x : {-1.f, -2.f, 0.1f, NAN}) { auto m = dm1; m[3] = x; auto w = v; w.dm1 = m.data(); REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "dm1 of direction 1, mirror 1")); }
  // footprints: direction 0 on mirror 1 (no cone): 83 + off <= 267
  { auto o = off; o[2] = 184.5f; auto w = v; w.off = o.data(); REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "the footprint of direction 0 leaves mirror 1")); }
  { auto o = off; o[2] = 184.f; auto w = v; w.off = o.data(); REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 0); }
  // ... and direction 2 on mirror 0 through its cone: 0 + off - 0.075 * (-41.5) >= 0
  { auto o = off; o[8] = -3.2f; auto w = v; w.off = o.data(); REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 1 && has(err, "the footprint of direction 2 leaves mirror 0")); }
  { auto o = off; o[8] = -3.1f; auto w = v; w.off = o.data(); REQUIRE(mcao_validate_add(&w, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 0, known, err) == 0); }
  REQUIRE(mcao_validate_add(&v, planes, 3, n, n, pd, 2, dims, 4, 2, 3, 0, known, err) == 1 && has(err, "mcao_add: environments"));
  REQUIRE(mcao_validate_add(&v, planes, 3, n, n, pd, 2, dims, 4, 0, 4, 3, known, err) == 1 && has(err, "unknown flags 3"));
  REQUIRE(mcao_validate_add(&v, planes, 3, n, n, pd, 2, dims, 110000, 0, 4, 0, known, err) == 1 && has(err, "2^31"));
  // the pupil grid
  { std::vector<float> o1 = {50.f, 50.f, 94.f, 94.f}, z = {0.f, 0.f}; aomarl_mcao_view w = {1, o1.data(), z.data()};
    REQUIRE(mcao_validate_add(&w, planes, 1, pd, n, pd, 2, dims, 4, 0, 4, known, known, err) == 0); }

  // ---- the slots and the offset table
  REQUIRE(mcao_slots(1) == 1 && mcao_slots(2) == 2 && mcao_slots(3) == 4 && mcao_slots(4) == 4 && mcao_slots(5) == 8 && mcao_slots(8) == 8);
  const McaoAddArgs a = mcao_add_args(&v, 2);
  for (int k = 0; k < AOMARL_MCAO_MAX_DIRS; k++)
    for (int m = 0; m < 2; m++) {
      REQUIRE(a.ox[m][k] == (k < 3 ? off[2 * (k * 2 + m)] : 0.f) && a.oy[m][k] == (k < 3 ? off[2 * (k * 2 + m) + 1] : 0.f));
      REQUIRE(a.dm1[m][k] == (k < 3 ? dm1[k * 2 + m] : 0.f));
    }
  { std::vector<float> o1 = {50.f, 51.f}, z = {-0.1f}; aomarl_mcao_view w = {1, o1.data(), z.data()};      // one mirror: the second row stays zero
    const McaoAddArgs b = mcao_add_args(&w, 1);
    REQUIRE(b.ox[0][0] == 50.f && b.oy[0][0] == 51.f && b.dm1[0][0] == -0.1f && b.ox[1][0] == 0.f && b.dm1[1][0] == 0.f); }

  // ---- the plan of the shape launch
  const McaoPlan p = mcao_plan(dims, 2);
  REQUIRE(p.nmirrors == 2 && p.tx[0] == 6 && p.tx[1] == 9 && p.first[0] == 0 && p.first[1] == 36 && p.first[2] == 36 + 81);
  const McaoPlan p1 = mcao_plan(dims + 1, 1);
  REQUIRE(p1.nmirrors == 1 && p1.tx[0] == 9 && p1.first[1] == 81 && p1.tx[1] == 0);

  // ---- a field that sees the mirrors: 20 directions (two launches), natural stars
  const int T = 20;
  std::vector<float> foff(2 * T * 2), fz(T * 2, 0.f);
  for (int k = 0; k < T; k++) { foff[4 * k] = 50.f + k; foff[4 * k + 1] = 50.f - 0.5f * k; foff[4 * k + 2] = 94.f + 2.f * k; foff[4 * k + 3] = 94.f; }
  aomarl_mcao_view fv = {T, foff.data(), fz.data()};
  REQUIRE(mcao_validate_attach(&fv, T, 2, dims, pd, err) == 0);
  REQUIRE(mcao_validate_attach(&fv, T - 1, 2, dims, pd, err) == 1 && has(err, "the view has 20 directions, the field 19"));
  REQUIRE(mcao_validate_attach(nullptr, T, 2, dims, pd, err) == 1 && has(err, "field_attach_mirrors: null view"));
  { auto z = fz; z[7] = -0.1f; auto w = fv; w.dm1 = z.data(); REQUIRE(mcao_validate_attach(&w, T, 2, dims, pd, err) == 1 && has(err, "dm1 of direction 3, mirror 1 = -0.1: a science direction is a natural star")); }
  { auto o = foff; o[4 * 19] = 101.f; auto w = fv; w.off = o.data(); REQUIRE(mcao_validate_attach(&w, T, 2, dims, pd, err) == 1 && has(err, "the footprint of direction 19 leaves mirror 0")); }
  { auto o = foff; o[9] = NAN; auto w = fv; w.off = o.data(); REQUIRE(mcao_validate_attach(&w, T, 2, dims, pd, err) == 1 && has(err, "off of direction 2, mirror 0 is not finite")); }
  FieldMirArgs base;
  memset(&base, 0, sizeof(base));
  base.planes = planes; base.nmirrors = 2; base.stride = 268 * 268; base.dim[0] = 180; base.dim[1] = 268;
  const std::vector<FieldLaunch> plan = field_plan(T);
  REQUIRE(plan.size() == 2 && plan[1].first == 16 && plan[1].count == 4);
  for (const FieldLaunch &L : plan) {
    const FieldMirArgs ma = field_mir_args(base, foff.data(), L);
    REQUIRE(ma.planes == planes && ma.nmirrors == 2 && ma.stride == 268 * 268 && ma.dim[1] == 268);
    for (int k = 0; k < AOMARL_FIELD_MAX_DIRS; k++)
      for (int m = 0; m < 2; m++) {
        const bool in = k < L.count;
        REQUIRE(ma.ox[m][k] == (in ? foff[2 * ((L.first + k) * 2 + m)] : 0.f));
        REQUIRE(ma.oy[m][k] == (in ? foff[2 * ((L.first + k) * 2 + m) + 1] : 0.f));
      }
  }
  printf("mcao_host_check: ok\n");
  return 0;
}
