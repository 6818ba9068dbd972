// field_host_check.cpp -- a stand-alone host program around the host half of the science field (aomarl_field_host.h: the
// validation of the desc and of the calls, the plan of the launches, the kernels' offset table), meant to be built with the
// address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o field_host_check field_host_check.cpp
// No GPU, no HIP.  Exit status 0: all held.
#include "aomarl_field_host.h"

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main() {
  std::string err;
  // a 160-pixel pupil on a 168-pixel array, three screens, a stack array (176) and a tip-tilt mirror (168) in the pupil
  FieldSys sy;
  memset(&sy, 0, sizeof(sy));
  sy.nlayers = 3; sy.dims[0] = 172; sy.dims[1] = 184; sy.dims[2] = 210;
  sy.pupdiam = 160; sy.hw = 8; sy.ndm = 2;
  sy.dm_dim[0] = 176; sy.dm_txo[0] = sy.dm_tyo[0] = 8.f;
  sy.dm_dim[1] = 168; sy.dm_txo[1] = sy.dm_tyo[1] = 4.f;
  const int nl = 3, T = 2;
  std::vector<float> off = {6.f, 6.f, 12.f, 12.f, 25.f, 25.f, 6.f, 6.f, 18.25f, 12.f, 43.5f, 25.f};
  aomarl_field_desc ok = {T, nl, off.data(), 1.f / 1.65f};
  void *slot = &err;
  REQUIRE(field_validate_desc(&ok, sy, 4, slot, err) == 0);
  REQUIRE(field_validate_desc(nullptr, sy, 4, slot, err) == 1 && has(err, "null desc"));
  REQUIRE(field_validate_desc(&ok, sy, 4, nullptr, err) == 1 && has(err, "null output"));
  for (int v : {0, -3}) { auto d = ok; d.ndir = v; REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 1 && has(err, "at least one direction")); }
  { auto d = ok; d.nlayers = 2; REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 1 && has(err, "offsets for 2 layers, the context has 3")); }
  { auto d = ok; d.off = nullptr; REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 1 && has(err, "null off")); }
  for (int v : {0, -1}) REQUIRE(field_validate_desc(&ok, sy, v, slot, err) == 1 && has(err, "environments: at least one"));
  for (float v : {0.f, -1.f, NAN, INFINITY}) { auto d = ok; d.inv_lambda = v; REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 1 && has(err, "inv_lambda")); }
  for (int v : {0, 129}) { auto s2 = sy; s2.hw = v; REQUIRE(field_validate_desc(&ok, s2, 4, slot, err) == 1 && has(err, "strehl_halfwin")); }
  REQUIRE(field_validate_desc(&ok, sy, 50000, slot, err) == 1 && has(err, "2^31"));
  { std::vector<float> big((size_t)2 * nl * 30000, 6.f); aomarl_field_desc d = {30000, nl, big.data(), 1.f};
    REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 1 && has(err, "2^31")); }
  for (float v : {NAN, INFINITY}) { auto o = off; o[9] = v; auto d = ok; d.off = o.data(); REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 1 && has(err, "off of direction 1, layer 1 is not finite")); }
  { auto o = off; o[10] = 50.5f; auto d = ok; d.off = o.data();      // 159 + 50.5 > 209
    REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 1 && has(err, "footprint of direction 1 leaves screen 2")); }
  { auto o = off; o[10] = 50.f; auto d = ok; d.off = o.data(); REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 0); }
  { auto o = off; o[3] = -0.25f; auto d = ok; d.off = o.data();
    REQUIRE(field_validate_desc(&d, sy, 4, slot, err) == 1 && has(err, "footprint of direction 0 leaves screen 1")); }
  { auto s2 = sy; s2.dm_txo[0] = 11.7f; REQUIRE(field_validate_desc(&ok, s2, 4, slot, err) == 1 && has(err, "mirror 0 is not in the pupil") && has(err, "altitude")); }
  { auto s2 = sy; s2.dm_tyo[1] = 3.f; REQUIRE(field_validate_desc(&ok, s2, 4, slot, err) == 1 && has(err, "mirror 1 is not in the pupil")); }

  // ---- the calls
  REQUIRE(field_validate_call("field_observe", 4, 4, 0, 4, 3, 3, err) == 0);
  REQUIRE(field_validate_call("field_observe", 4, 4, 1, 3, 1, 3, err) == 0);
  REQUIRE(field_validate_call("field_observe", 4, 3, 0, 3, 3, 3, err) == 1 && has(err, "field_observe: the field has 4 environments, the state 3"));
  REQUIRE(field_validate_call("field_observe", 4, 4, 2, 3, 3, 3, err) == 1 && has(err, "field_observe: environments 2 .. +3 of 4"));
  REQUIRE(field_validate_call("field_trace", 4, 4, -1, 2, 3, 15, err) == 1 && has(err, "field_trace: environments"));
  REQUIRE(field_validate_call("field_reset", 4, 4, 0, 0, 0, 0, err) == 1 && has(err, "field_reset: environments"));
  REQUIRE(field_validate_call("field_observe", 4, 4, 0, 4, 4, 3, err) == 1 && has(err, "unknown flags 4"));
  REQUIRE(field_validate_call("field_trace", 4, 4, 0, 4, 16, 15, err) == 1 && has(err, "unknown flags 16"));
  REQUIRE(field_validate_call("field_trace", 4, 4, 0x7fffffff, 0x7fffffff, 0, 15, err) == 1 && has(err, "environments"));

  // ---- the plan: every direction exactly once, in order, at most 16 per launch
  for (int ndir : {1, 3, 15, 16, 17, 32, 33, 100}) {
    const std::vector<FieldLaunch> p = field_plan(ndir);
    REQUIRE((int)p.size() == (ndir + AOMARL_FIELD_MAX_DIRS - 1) / AOMARL_FIELD_MAX_DIRS);
    int next = 0;
    for (const FieldLaunch &L : p) {
      REQUIRE(L.first == next && L.count >= 1 && L.count <= AOMARL_FIELD_MAX_DIRS && L.count <= field_chunk(ndir));
      next += L.count;
    }
    REQUIRE(next == ndir);
  }
  REQUIRE(field_chunk(3) == 3 && field_chunk(16) == 16 && field_chunk(17) == 16);
  // the kernel instantiation's direction slots: the next power of two, never below the launch's count nor above 16
  for (int k = 1; k <= AOMARL_FIELD_MAX_DIRS; k++) {
    const int kt = field_slots(k);
    REQUIRE(kt >= k && kt < 2 * k && kt <= AOMARL_FIELD_MAX_DIRS && (kt & (kt - 1)) == 0);
  }
  REQUIRE(field_slots(1) == 1 && field_slots(3) == 4 && field_slots(9) == 16);

  // ---- the offset table: [layer][direction of the launch], untouched entries zero, the remainders added per layer
  {
    const int ndir = 17;
    std::vector<float> o17((size_t)2 * nl * ndir);
    for (size_t i = 0; i < o17.size(); i++) o17[i] = 0.25f * (float)i;
    const std::vector<FieldLaunch> p = field_plan(ndir);
    const float fx[3] = {0.5f, 0.f, 0.125f}, fy[3] = {0.f, 0.75f, 0.25f};
    for (const FieldLaunch &L : p) {
      const FieldArgs a = field_args(o17.data(), nl, L, nullptr, nullptr), b = field_args(o17.data(), nl, L, fx, fy);
      for (int l = 0; l < FIELD_MAX_LAYERS; l++)
        for (int k = 0; k < AOMARL_FIELD_MAX_DIRS; k++) {
          const bool live = l < nl && k < L.count;
          const float wx = live ? o17[2 * ((size_t)(L.first + k) * nl + l)] : 0.f, wy = live ? o17[2 * ((size_t)(L.first + k) * nl + l) + 1] : 0.f;
          REQUIRE(a.ox[l][k] == wx && a.oy[l][k] == wy);
          REQUIRE(b.ox[l][k] == (live ? wx + fx[l] : 0.f) && b.oy[l][k] == (live ? wy + fy[l] : 0.f));
        }
    }
    // direction 16 alone in a field of its own: the same numbers in slot 0
    const FieldArgs whole = field_args(o17.data(), nl, p[1], nullptr, nullptr);
    const FieldArgs own = field_args(o17.data() + (size_t)2 * nl * 16, nl, field_plan(1)[0], nullptr, nullptr);
    REQUIRE(memcmp(&whole, &own, sizeof(whole)) == 0);
  }
  printf("field_host_check: ok\n");
  return 0;
}
