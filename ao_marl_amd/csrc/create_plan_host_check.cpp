// create_plan_host_check.cpp -- a stand-alone host program around aomarl_create_plan_host.h (what aomarl_create derives
// from a descriptor), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o create_plan_host_check create_plan_host_check.cpp
// No GPU, no HIP.  It generates small systems of its own (an LCG, pupils of 32, 48 and 64 pixels), plans each of them,
// and checks every table of an accepted one against a brute-force definition written here, not shared with the header;
// then one descriptor per refusal.  Exit status 0: all held, and the line "create_plan_host_check: ok (<count> cases)".
//     create_plan_host_check --table   also prints one block per case: accepted or refused (with the message), every scalar
//                                      of DevSys and of the host values, and per table its name, byte count, FNV-1a-64 and
//                                      the DevSys fields it is stored in (tests/test_create_plan.py compares it with
//                                      tests/golden/create_plans.txt)
// Everything below works on an Outcome, not on the plan: the golden was recorded by building this file with
// -DCREATE_OUTCOME_EXTERN around the function the plan replaced (outcome() defined there).  psf_tw_h is not the
// plan's: the executor forms it from psf_tw_f, and its line here is this file's own float-to-half rounding (f2h).
#include "aomarl_create_plan_host.h"
#include <stddef.h>
#include <stdlib.h>
#include <map>

#define REQUIRE(c)                                                                                        \
  do {                                                                                                    \
    if (!(c)) { fprintf(stderr, "%s:%d: [%s] %s failed\n", __FILE__, __LINE__, g_case, #c); exit(1); }    \
  } while (0)
static const char *g_case = "";

struct Tab { std::string name; std::vector<unsigned char> bytes; std::vector<size_t> slots; };
struct Outcome {
  bool ok = false;
  std::string msg;
  DevSys sys;
  CreateHost host;
  bool layout = false;
  std::vector<Tab> tabs;
};

// ---- float <-> half, round to nearest even (the executor's (_Float16)v)
static uint16_t f2h(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  const int e = (int)((x >> 23) & 0xFF) - 127;
  uint32_t m = x & 0x7FFFFFu;
  if (e == 128) return (uint16_t)(sign | 0x7C00u | (m ? 0x200u : 0u));
  if (e > 15) return (uint16_t)(sign | 0x7C00u);
  if (e < -25) return (uint16_t)sign;
  int shift = 13;
  uint32_t base = (uint32_t)(e + 15) << 10;
  if (e < -14) { m |= 0x800000u; shift = -1 - e; base = 0; }       // subnormal half
  uint32_t h = base + (m >> shift);
  const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (h & 1))) h++;
  return (uint16_t)(sign | h);
}
static float h2f(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 1023;
  const float v = e == 0 ? ldexpf((float)m, -24) : ldexpf((float)(m + 1024), e - 25);
  return (h & 0x8000) ? -v : v;
}

#ifdef CREATE_OUTCOME_EXTERN
Outcome outcome(const aomarl_desc *d);
#else
static Outcome outcome(const aomarl_desc *d) {
  Outcome o;
  CreatePlan P;
  o.ok = create_plan(d, P);
  o.msg = P.msg;
  if (!o.ok) return o;
  o.sys = P.sys; o.host = P.host; o.layout = P.production_layout;
  for (size_t i = 0; i < P.tables.size(); i++) {
    const CreateTable &T = P.tables[i];
    const unsigned char *b = (const unsigned char *)T.data();
    if ((int)i == P.psf_operand) {
      Tab h;
      h.name = "psf_tw_h"; h.slots.push_back(offsetof(DevSys, psf_tw_h));
      std::vector<uint16_t> tw(T.bytes / 4 * 2);
      const float *twf = (const float *)T.data();
      for (size_t q = 0; q < T.bytes / 16; q++)
        for (int j = 0; j < 4; j++) {
          const float v = twf[q * 4 + j];
          const uint16_t hi = f2h(v);
          tw[q * 8 + j] = hi; tw[q * 8 + 4 + j] = f2h(v - h2f(hi));
        }
      h.bytes.assign((unsigned char *)tw.data(), (unsigned char *)tw.data() + tw.size() * 2);
      o.tabs.push_back(h);
    }
    o.tabs.push_back(Tab{T.name, std::vector<unsigned char>(b, b + T.bytes), T.slots});
  }
  for (int c = 0; c < P.host.nclass; c++) REQUIRE(P.tables[P.ab_table[c]].name.find(".AB") != std::string::npos);
  return o;
}
#endif

// ---- the pointer fields of DevSys by name
static std::vector<std::pair<std::string, size_t>> fields() {
  std::vector<std::pair<std::string, size_t>> f;
#define F(x) f.push_back({#x, offsetof(DevSys, x)})
  F(mpupil); F(spupil); F(phasemap); F(sub_xy); F(halfxy); F(binmap); F(flux); F(validx); F(validy); F(psf_tw);
  F(stripe_order); F(tile_info); F(lit_info); F(lit_count); F(pair_info); F(pair_count); F(tile_mask); F(psf_tw_h);
  F(psf_tw_f); F(qf_tab); F(tt_pk);
#undef F
  for (int l = 0; l < AOMARL_MAX_LAYERS; l++) {
    const size_t b = offsetof(DevSys, layers) + l * sizeof(DevLayer);
    const std::string p = "layers[" + std::to_string(l) + "].";
    f.push_back({p + "istx", b + offsetof(DevLayer, istx)}); f.push_back({p + "isty", b + offsetof(DevLayer, isty)});
    f.push_back({p + "istT", b + offsetof(DevLayer, istT)}); f.push_back({p + "AB", b + offsetof(DevLayer, AB)});
    f.push_back({p + "ABt", b + offsetof(DevLayer, ABt)});
  }
  for (int k = 0; k < AOMARL_MAX_DMS; k++) {
    const size_t b = offsetof(DevSys, dms) + k * sizeof(DevDm);
    const std::string p = "dms[" + std::to_string(k) + "].";
    f.push_back({p + "influ", b + offsetof(DevDm, influ)}); f.push_back({p + "influpos", b + offsetof(DevDm, influpos)});
    f.push_back({p + "ninflu", b + offsetof(DevDm, ninflu)}); f.push_back({p + "influstart", b + offsetof(DevDm, influstart)});
    f.push_back({p + "grid", b + offsetof(DevDm, grid)}); f.push_back({p + "prof", b + offsetof(DevDm, prof)});
  }
  return f;
}
static std::string field_name(size_t off) {
  static const std::vector<std::pair<std::string, size_t>> f = fields();
  for (auto &e : f) if (e.second == off) return e.first;
  return "?";
}

// ---- the generated systems
struct Lcg {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  float unit() { return (float)(next() & 0xFFFFFF) / 16777216.0f - 0.5f; }
};

enum Pupil { FULL, DISC, GREY };
enum DmKind { DM_P16, DM_P12, DM_DIFFER, DM_DOUBLE, DM_FINE };
struct Geo {
  int pd = 32, pad = 0;
  Pupil pupil = FULL;
  int nlayers = 1;
  int dim[3] = {96, 96, 96}, ns[3] = {40, 40, 40}, share[3] = {0, 0, 1};
  float wox[3] = {4, 6, 8}, woy[3] = {5, 7, 9};
  float tdx[3] = {0, 0, 0};              // tar_xoff - (wfs_xoff + pad)
  DmKind dm = DM_P16;
  bool tt_first = false;
  int hw = 8, npsf = 256;
  int max_side = 1 << 20;                // actuators per axis at most
};

struct Sys {
  aomarl_desc d;
  std::vector<float> mpupil, spupil, halfxy, flux, A[3], B[3], influ, tt;
  std::vector<int32_t> phasemap, binmap, vx, vy, influpos, ninflu, influstart;
  std::vector<uint32_t> istx[3], isty[3];
  std::vector<int> tile_of_sub;          // r * nt + t
  std::vector<int> act_x, act_y;         // top-left pixel of every stack-array actuator's patch
  int pitch = 0;
};

static void build(const Geo &g, Sys &S) {
  Lcg R{0x5DEECE66Dull + (uint64_t)g.pd * 131 + (uint64_t)g.dm * 17 + (uint64_t)g.nlayers};
  aomarl_desc &d = S.d;
  memset(&d, 0, sizeof(d));
  d.abi_version = AOMARL_ABI_VERSION;
  const int pd = g.pd, n = pd + 2 * g.pad, nt = pd / 16;
  d.n = n; d.pupdiam = pd;
  S.spupil.assign((size_t)pd * pd, 0.f);
  for (int y = 0; y < pd; y++)
    for (int x = 0; x < pd; x++) {
      bool lit = true;
      if (g.pupil == DISC) lit = (x - 24) * (x - 24) + (y - 24) * (y - 24) <= 400;
      S.spupil[(size_t)y * pd + x] = lit ? 1.f : 0.f;
    }
  if (g.pupil == GREY) S.spupil[(size_t)5 * pd + 7] = 0.5f;
  S.mpupil.assign((size_t)n * n, 0.f);
  for (int y = 0; y < pd; y++)
    for (int x = 0; x < pd; x++) S.mpupil[(size_t)(y + g.pad) * n + x + g.pad] = S.spupil[(size_t)y * pd + x];
  // a sub-aperture on every tile that is at least half lit
  S.tile_of_sub.clear();
  for (int r = 0; r < nt; r++)
    for (int t = 0; t < nt; t++) {
      int lit = 0;
      for (int yy = 0; yy < 16; yy++)
        for (int xx = 0; xx < 16; xx++) lit += S.spupil[(size_t)(16 * r + yy) * pd + 16 * t + xx] != 0.f;
      if (lit >= 128) S.tile_of_sub.push_back(r * nt + t);
    }
  const int nv = (int)S.tile_of_sub.size();
  d.nvalid = nv; d.pdiam = 16; d.nfft = 64; d.npix = 16; d.nrebin = 2; d.nxsub = nt;
  S.phasemap.assign((size_t)256 * nv + 1, 0);
  S.vx.assign(nv + 1, 0); S.vy.assign(nv + 1, 0); S.flux.assign(nv + 1, 0.f);
  for (int i = 0; i < nv; i++) {
    const int r = S.tile_of_sub[i] / nt, t = S.tile_of_sub[i] % nt;
    const int p0 = (g.pad + 16 * r) * n + g.pad + 16 * t;
    for (int k = 0; k < 256; k++) S.phasemap[(size_t)k * nv + i] = p0 + (k % 16) + n * (k / 16);
    S.vx[i] = 16 * t; S.vy[i] = 16 * r; S.flux[i] = 0.5f + R.unit() * 0.25f;
  }
  S.halfxy.resize(256);
  for (int k = 0; k < 256; k++) S.halfxy[k] = (float)(M_PI * (double)((k % 16) + (k / 16)) / 64.0);
  S.binmap.resize(4 * 256);
  for (int r = 0; r < 4; r++)
    for (int px = 0; px < 256; px++) {
      const int Y = px / 16, X = px % 16;
      S.binmap[r * 256 + px] = ((2 * Y - 16 + r / 2 + 64) % 64) * 64 + (2 * X - 16 + r % 2 + 64) % 64;
    }
  d.mpupil = S.mpupil.data(); d.spupil = S.spupil.data(); d.phasemap = S.phasemap.data(); d.halfxy = S.halfxy.data();
  d.binmap = S.binmap.data(); d.flux = S.flux.data(); d.validsubsx = S.vx.data(); d.validsubsy = S.vy.data();
  d.nphot = 100.f; d.wfs_lambda = 0.5f; d.noise = 0.25f; d.cog_offset = 7.5f; d.cog_scale = 0.125f; d.subapd = 0.5f;
  // layers
  d.nlayers = g.nlayers;
  for (int l = 0; l < g.nlayers; l++) {
    aomarl_layer_desc &L = d.layers[l];
    const int dim = g.dim[l], ns = g.ns[l];
    int same = -1;
    for (int m = 0; m < l; m++) if (g.share[m] == g.share[l]) same = m;
    if (same >= 0) { REQUIRE(g.dim[same] == dim && g.ns[same] == ns); L.A = S.A[same].data(); L.B = S.B[same].data(); }
    else {
      S.A[l].resize((size_t)dim * ns); S.B[l].resize((size_t)dim * dim);
      for (float &v : S.A[l]) v = R.unit();
      for (float &v : S.B[l]) v = R.unit() * 8.f;
      L.A = S.A[l].data(); L.B = S.B[l].data();
    }
    S.istx[l].resize(ns); S.isty[l].resize(ns);
    for (int k = 0; k < ns; k++) { S.istx[l][k] = R.next() % (uint32_t)(dim * dim); S.isty[l][k] = R.next() % (uint32_t)(dim * dim); }
    L.dim = dim; L.nstencil = ns; L.istx = S.istx[l].data(); L.isty = S.isty[l].data();
    L.deltax = 0.25f * (l + 1); L.deltay = -0.125f * (l + 1); L.amplitude = 1.5f + l;
    L.wfs_xoff = g.wox[l]; L.wfs_yoff = g.woy[l];
    L.tar_xoff = g.wox[l] + g.pad + g.tdx[l]; L.tar_yoff = g.woy[l] + g.pad;
  }
  // mirrors: a stack array on a lattice and a tip-tilt
  const int mdim = n + 16;
  int pitch = 16, ss = 32;
  if (g.dm == DM_P12) { pitch = 12; ss = 24; }
  if (g.dm == DM_FINE) { pitch = 4; ss = 16; }
  S.pitch = pitch;
  S.act_x.clear(); S.act_y.clear();
  for (int y = -8; y < mdim && y < -8 + g.max_side * pitch; y += pitch)
    for (int x = -8; x < mdim && x < -8 + g.max_side * pitch; x += pitch) { S.act_x.push_back(x); S.act_y.push_back(y); }
  if (g.dm == DM_DOUBLE) { S.act_x.push_back(S.act_x[3]); S.act_y.push_back(S.act_y[3]); }
  const int na = (int)S.act_x.size();
  std::vector<float> prof(ss);
  for (int t = 0; t < ss; t++) {           // (a bell from + * / alone: the same bits with every libm)
    const float u = (float)(2 * t - ss + 1) / (float)ss;
    prof[t] = 0.25f + 0.75f / (1.f + 4.f * u * u);
  }
  S.influ.resize((size_t)na * ss * ss);
  for (int a = 0; a < na; a++)
    for (int i = 0; i < ss; i++)
      for (int j = 0; j < ss; j++) S.influ[((size_t)a * ss + i) * ss + j] = prof[i] * prof[j] * ((g.dm == DM_DIFFER && a == 1) ? 1.5f : 1.f);
  S.ninflu.assign((size_t)mdim * mdim, 0); S.influstart.assign((size_t)mdim * mdim, 0);
  auto patch = [&](auto each) {            // every (pixel, sample) of every actuator's patch inside the support, by actuator
    for (int a = 0; a < na; a++)
      for (int aa = 0; aa < ss; aa++)
        for (int b = 0; b < ss; b++) {
          const int x = S.act_x[a] + b, y = S.act_y[a] + aa;
          if (x >= 0 && x < mdim && y >= 0 && y < mdim) each((size_t)y * mdim + x, (a * ss + aa) * ss + b);
        }
  };
  patch([&](size_t px, int) { S.ninflu[px]++; });
  size_t total = 0;
  for (size_t px = 0; px < (size_t)mdim * mdim; px++) { S.influstart[px] = (int32_t)total; total += S.ninflu[px]; }
  S.influpos.assign(total, 0);
  std::vector<int32_t> cursor(S.influstart);
  patch([&](size_t px, int pos) { S.influpos[cursor[px]++] = pos; });
  S.influpos.push_back(0);                 // (one spare entry: a refused case claims one more)
  S.tt.resize((size_t)mdim * mdim * 2);
  for (int y = 0; y < mdim; y++)
    for (int x = 0; x < mdim; x++) { S.tt[2 * ((size_t)y * mdim + x)] = (float)(x - mdim / 2) * 0.03125f; S.tt[2 * ((size_t)y * mdim + x) + 1] = (float)(y - mdim / 2) * 0.0625f; }
  d.ndm = 2;
  aomarl_dm_desc &Z = d.dms[g.tt_first ? 1 : 0], &T = d.dms[g.tt_first ? 0 : 1];
  Z.type = AOMARL_DM_PZT; Z.dim = mdim; Z.nact = na; Z.influsize = ss; Z.ninflupos = (int64_t)S.influpos.size() - 1;
  Z.influ = S.influ.data(); Z.influpos = S.influpos.data(); Z.ninflu = S.ninflu.data(); Z.influstart = S.influstart.data();
  T.type = AOMARL_DM_TT; T.dim = mdim; T.nact = 2; T.influ = S.tt.data();
  for (int k = 0; k < 2; k++) {
    d.dms[k].wfs_xoff = 8; d.dms[k].wfs_yoff = 8; d.dms[k].tar_xoff = 8 + g.pad; d.dms[k].tar_yoff = 8 + g.pad;
  }
  d.tar_lambda = 1.65f; d.npsf = g.npsf; d.strehl_halfwin = g.hw;
  d.nactu = na + 2; d.nslope = 2 * nv; d.gain = 0.4f; d.delay = 1.f;
}

// ---- the table
static uint64_t fnv(const void *p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char *)p)[i]; h *= 0x100000001b3ull; }
  return h;
}
static void print_outcome(const char *name, const Outcome &o) {
  printf("case %s\n", name);
  if (!o.ok) { printf("  refused: %s\n", o.msg.c_str()); return; }
  const DevSys &s = o.sys;
  printf("  accepted layout %d\n", o.layout ? 1 : 0);
  printf("  sys n %d pupdiam %d nvalid %d pdiam %d nfft %d npix %d nrebin %d nxsub %d nphot %a wfs_inv_lambda %a noise %a cog_offset %a "
         "cog_scale %a subapd %a nlayers %d ndm %d\n", s.n, s.pupdiam, s.nvalid, s.pdiam, s.nfft, s.npix, s.nrebin, s.nxsub, s.nphot,
         s.wfs_inv_lambda, s.noise, s.cog_offset, s.cog_scale, s.subapd, s.nlayers, s.ndm);
  for (int l = 0; l < s.nlayers; l++) {
    const DevLayer &L = s.layers[l];
    printf("  layer %d dim %d ns %d screen_off %lld ldab %d ldt %d amp %a off %a %a %a %a int %d %d %d %d\n", l, L.dim, L.ns, L.screen_off,
           L.ldab, L.ldt, L.amp, L.wxo, L.wyo, L.txo, L.tyo, L.wox, L.woy, L.tox, L.toy);
  }
  for (int k = 0; k < s.ndm; k++) {
    const DevDm &D = s.dms[k];
    printf("  dm %d type %d dim %d nact %d ss %d shape_off %lld com_off %d off %a %a %a %a int %d %d %d %d sep %d pitch %d i1min %d j1min %d "
           "gw %d gh %d\n", k, D.type, D.dim, D.nact, D.ss, D.shape_off, D.com_off, D.wxo, D.wyo, D.txo, D.tyo, D.wox, D.woy, D.tox, D.toy,
           D.sep, D.pitch, D.i1min, D.j1min, D.gw, D.gh);
  }
  printf("  sys tar_inv_lambda %a npsf %d hw %d ref_peak %a nactu %d nslope %d wfs_all_int %d tar_all_int %d screen_stride %lld "
         "shape_stride %lld fused_ok %d ntiles %d otf_ok %d otf_nb %d otf_tpn %d otf_gx0 %d otf_gy0 %d otf_xoff %d otf_yoff %d otf_latw %d\n",
         s.tar_inv_lambda, s.npsf, s.hw, s.ref_peak, s.nactu, s.nslope, s.wfs_all_int, s.tar_all_int, s.screen_stride, s.shape_stride,
         s.fused_ok, s.ntiles, s.otf_ok, s.otf_nb, s.otf_tpn, s.otf_gx0, s.otf_gy0, s.otf_xoff, s.otf_yoff, s.otf_latw);
  const CreateHost &H = o.host;
  printf("  host");
  for (int l = 0; l < s.nlayers; l++) printf(" [%d dim %d ns %d abclass %d delta %a %a]", l, H.dim[l], H.ns[l], H.abclass[l], H.deltax[l], H.deltay[l]);
  printf(" nclass %d maxdim %d maxK %d small_ok %d gain %a delay %a\n", H.nclass, H.maxdim, H.maxK, H.small_ok ? 1 : 0, H.gain, H.delay);
  printf("  host h_grid %zu %016llx h_prof %zu %016llx h_spupil %zu %016llx h_tt %zu %016llx\n",
         H.h_grid.size() * 4, (unsigned long long)fnv(H.h_grid.data(), H.h_grid.size() * 4), H.h_prof.size() * 4,
         (unsigned long long)fnv(H.h_prof.data(), H.h_prof.size() * 4), H.h_spupil.size() * 4,
         (unsigned long long)fnv(H.h_spupil.data(), H.h_spupil.size() * 4), H.h_tt.size() * 4, (unsigned long long)fnv(H.h_tt.data(), H.h_tt.size() * 4));
  for (const Tab &t : o.tabs) {
    printf("  table %s %zu %016llx ->", t.name.c_str(), t.bytes.size(), (unsigned long long)fnv(t.bytes.data(), t.bytes.size()));
    for (size_t off : t.slots) printf(" %s", field_name(off).c_str());
    printf("\n");
  }
}

// ---- invariants of an accepted case, from the descriptor alone
struct Want { int fused, otf, sep, small_ok, wfs_int; };

template <typename T>
static const T *tab(const Outcome &o, const std::string &name, size_t count) {
  for (const Tab &t : o.tabs)
    for (size_t off : t.slots)
      if (field_name(off) == name) { REQUIRE(t.bytes.size() == count * sizeof(T)); return (const T *)t.bytes.data(); }
  REQUIRE(count == 0);
  return nullptr;
}
static bool has_tab(const Outcome &o, const std::string &name) {
  for (const Tab &t : o.tabs)
    for (size_t off : t.slots) if (field_name(off) == name) return true;
  return false;
}

static void check_accepted(const Sys &S, const Outcome &o, const Want &w) {
  const aomarl_desc &d = S.d;
  const DevSys &s = o.sys;
  const int n = d.n, pd = d.pupdiam, pad = (n - pd) / 2, nv = d.nvalid;
  // every slot is a pointer field, named once; the table's name is its first field
  std::map<size_t, int> seen;
  for (const Tab &t : o.tabs) {
    REQUIRE(!t.slots.empty() && !t.bytes.empty() && t.name == field_name(t.slots[0]));
    for (size_t off : t.slots) { REQUIRE(field_name(off) != "?"); REQUIRE(seen[off]++ == 0); }
  }
  // pointers of the plan's DevSys are null
  for (auto &f : fields()) { const void *p; memcpy(&p, (const char *)&s + f.second, sizeof(p)); REQUIRE(p == nullptr); }
  // pass-through tables, byte for byte; sizes as the kernels index them
  REQUIRE(memcmp(tab<float>(o, "mpupil", (size_t)n * n), d.mpupil, (size_t)n * n * 4) == 0);
  REQUIRE(memcmp(tab<float>(o, "spupil", (size_t)pd * pd), d.spupil, (size_t)pd * pd * 4) == 0);
  REQUIRE(o.host.h_spupil.size() == (size_t)pd * pd && memcmp(o.host.h_spupil.data(), d.spupil, (size_t)pd * pd * 4) == 0);
  if (nv) {
    REQUIRE(memcmp(tab<int32_t>(o, "phasemap", (size_t)256 * nv), d.phasemap, (size_t)256 * nv * 4) == 0);
    REQUIRE(memcmp(tab<float>(o, "flux", nv), d.flux, (size_t)nv * 4) == 0);
    REQUIRE(memcmp(tab<int32_t>(o, "validx", nv), d.validsubsx, (size_t)nv * 4) == 0);
    REQUIRE(memcmp(tab<int32_t>(o, "validy", nv), d.validsubsy, (size_t)nv * 4) == 0);
    const int32_t *sub = tab<int32_t>(o, "sub_xy", nv);
    for (int i = 0; i < nv; i++) REQUIRE((sub[i] & 0xFFFF) == d.phasemap[i] % n && (sub[i] >> 16) == d.phasemap[i] / n);
  }
  REQUIRE(memcmp(tab<int32_t>(o, "binmap", 1024), d.binmap, 4096) == 0);
  const float *hx = tab<float>(o, "halfxy", 256);
  for (int k = 0; k < 256; k++) REQUIRE(fabs((double)hx[k] - (double)((k % 16) + (k / 16)) / 128.0) < 1e-7);
  // layers: prefix sums, stencils, [A | B] and its transpose, classes
  long long off = 0;
  int nclass = 0, maxdim = 0, maxK = 0, wint = 1, tint = 1;
  bool small = true;
  for (int l = 0; l < d.nlayers; l++) {
    const aomarl_layer_desc &L = d.layers[l];
    const DevLayer &D = s.layers[l];
    const std::string p = "layers[" + std::to_string(l) + "].";
    REQUIRE(D.dim == L.dim && D.ns == L.nstencil && D.screen_off == off && o.host.dim[l] == L.dim && o.host.ns[l] == L.nstencil);
    off += (long long)L.dim * (L.dim + 56);
    maxdim = std::max(maxdim, L.dim); maxK = std::max(maxK, L.dim + L.nstencil);
    const uint32_t *ix = tab<uint32_t>(o, p + "istx", L.nstencil), *iy = tab<uint32_t>(o, p + "isty", L.nstencil), *iT = tab<uint32_t>(o, p + "istT", L.nstencil);
    for (int k = 0; k < L.nstencil; k++) {
      REQUIRE((ix[k] & 0xFFFF) + (ix[k] >> 16) * (uint32_t)L.dim == L.istx[k] && (iy[k] & 0xFFFF) + (iy[k] >> 16) * (uint32_t)L.dim == L.isty[k]);
      REQUIRE((iT[k] & 0xFFFF) == (ix[k] >> 16) && (iT[k] >> 16) == (ix[k] & 0xFFFF));
    }
    int first = l;
    for (int m = l - 1; m >= 0; m--) if (d.layers[m].A == L.A && d.layers[m].B == L.B) first = m;
    if (first == l) nclass++;
    REQUIRE(o.host.abclass[l] == o.host.abclass[first] && (first < l || o.host.abclass[l] == nclass - 1));
    const int K = L.dim + L.nstencil;
    REQUIRE(D.ldab == ((K + 3) & ~3));
    const float *ab = tab<float>(o, p + "AB", (size_t)L.dim * D.ldab);
    REQUIRE(ab == tab<float>(o, "layers[" + std::to_string(first) + "].AB", (size_t)L.dim * D.ldab));
    for (int r = 0; r < L.dim; r++)
      for (int j = 0; j < D.ldab; j++)
        REQUIRE(ab[(size_t)r * D.ldab + j] == (j < L.nstencil ? L.A[(size_t)r * L.nstencil + j] : j < K ? L.B[(size_t)r * L.dim + j - L.nstencil] : 0.f));
    const bool fits = L.dim <= 256 && K <= 4096;
    REQUIRE(has_tab(o, p + "ABt") == fits && D.ldt == (fits ? (L.dim + 63) & ~63 : 0));
    if (fits) {
      const float *abt = tab<float>(o, p + "ABt", (size_t)K * D.ldt);
      for (int j = 0; j < K; j++)
        for (int r = 0; r < D.ldt; r++) REQUIRE(abt[(size_t)j * D.ldt + r] == (r < L.dim ? ab[(size_t)r * D.ldab + j] : 0.f));
    } else small = false;
    REQUIRE(D.wox == (int)L.wfs_xoff && D.tox == (int)L.tar_xoff && D.woy == (int)L.wfs_yoff && D.toy == (int)L.tar_yoff);
    if (L.wfs_xoff != floorf(L.wfs_xoff) || L.wfs_yoff != floorf(L.wfs_yoff)) wint = 0;
    if (L.tar_xoff != floorf(L.tar_xoff) || L.tar_yoff != floorf(L.tar_yoff)) tint = 0;
  }
  REQUIRE(s.screen_stride == off && o.host.nclass == nclass && o.host.maxdim == maxdim && o.host.maxK == maxK && o.host.small_ok == small);
  REQUIRE(s.wfs_all_int == wint && s.tar_all_int == tint && wint == w.wfs_int && (int)small == w.small_ok);
  // mirrors: prefix sums, the lattice
  long long soff = 0;
  int coff = 0;
  for (int k = 0; k < d.ndm; k++) {
    const aomarl_dm_desc &M = d.dms[k];
    const DevDm &D = s.dms[k];
    const std::string p = "dms[" + std::to_string(k) + "].";
    REQUIRE(D.shape_off == soff && D.com_off == coff && D.dim == M.dim && D.nact == M.nact);
    soff += M.type == AOMARL_DM_TT ? 4 : (long long)M.dim * M.dim;
    coff += M.nact;
    if (M.type == AOMARL_DM_TT) {
      REQUIRE(memcmp(tab<float>(o, p + "influ", (size_t)M.dim * M.dim * 2), M.influ, (size_t)M.dim * M.dim * 8) == 0);
      REQUIRE(D.sep == 0 && o.host.h_tt.size() == (k == 1 ? (size_t)M.dim * M.dim * 2 : 0));
      continue;
    }
    const int ss = M.influsize;
    REQUIRE(memcmp(tab<float>(o, p + "influ", (size_t)M.nact * ss * ss), M.influ, (size_t)M.nact * ss * ss * 4) == 0);
    REQUIRE(memcmp(tab<int32_t>(o, p + "influpos", (size_t)M.ninflupos), M.influpos, (size_t)M.ninflupos * 4) == 0);
    REQUIRE(memcmp(tab<int32_t>(o, p + "ninflu", (size_t)M.dim * M.dim), M.ninflu, (size_t)M.dim * M.dim * 4) == 0);
    REQUIRE(memcmp(tab<int32_t>(o, p + "influstart", (size_t)M.dim * M.dim), M.influstart, (size_t)M.dim * M.dim * 4) == 0);
    REQUIRE(D.sep == w.sep && has_tab(o, p + "grid") == (D.sep != 0) && has_tab(o, p + "prof") == (D.sep != 0));
    if (!D.sep) { REQUIRE(k != 0 || (o.host.h_grid.empty() && o.host.h_prof.empty())); continue; }
    const int32_t *grid = tab<int32_t>(o, p + "grid", (size_t)D.gw * D.gh);
    const float *prof = tab<float>(o, p + "prof", ss);
    if (k == 0) REQUIRE(o.host.h_grid.size() == (size_t)D.gw * D.gh && memcmp(o.host.h_grid.data(), grid, o.host.h_grid.size() * 4) == 0 &&
                        o.host.h_prof.size() == (size_t)ss && memcmp(o.host.h_prof.data(), prof, (size_t)ss * 4) == 0);
    std::vector<int> cell_of(M.nact, -1);
    for (int c = 0; c < D.gw * D.gh; c++)
      if (grid[c] != -1) { REQUIRE(grid[c] >= 0 && grid[c] < M.nact && cell_of[grid[c]] == -1); cell_of[grid[c]] = c; }
    float best = 0.f;
    for (int t = 0; t < ss; t++) best = std::max(best, M.influ[t * ss + t]);
    for (int a = 0; a < M.nact; a++) {
      REQUIRE(cell_of[a] >= 0);
      REQUIRE(D.i1min + D.pitch * (cell_of[a] % D.gw) == S.act_x[a] && D.j1min + D.pitch * (cell_of[a] / D.gw) == S.act_y[a]);
    }
    for (long long px = 0; px < (long long)M.dim * M.dim; px++)
      for (int t = 0; t < M.ninflu[px]; t++) {
        const int pos = M.influpos[M.influstart[px] + t], a = pos / (ss * ss), i = pos % (ss * ss) / ss, j = pos % ss;
        REQUIRE(fabsf(M.influ[pos] - prof[i] * prof[j]) <= 2e-6f * best);
        REQUIRE(D.i1min + D.pitch * (cell_of[a] % D.gw) + j == (int)(px % M.dim) && D.j1min + D.pitch * (cell_of[a] / D.gw) + i == (int)(px / M.dim));
      }
  }
  REQUIRE(s.shape_stride == soff && coff == d.nactu && s.nactu == d.nactu && s.nslope == 2 * nv);
  REQUIRE(o.layout == (d.ndm == 2 && d.dms[0].type == AOMARL_DM_PZT && d.dms[1].type == AOMARL_DM_TT && (d.nlayers == 1 || d.nlayers == 3)));
  // target
  const float *tw = tab<float>(o, "psf_tw", (size_t)d.npsf * 2);
  for (int j = 0; j < d.npsf; j++)
    REQUIRE(fabs(tw[2 * j] - cos(2.0 * M_PI * j / d.npsf)) <= 1.2e-7 && fabs(tw[2 * j + 1] - sin(2.0 * M_PI * j / d.npsf)) <= 1.2e-7);
  double sp = 0.;
  for (size_t q = 0; q < (size_t)pd * pd; q++) sp += d.spupil[q];
  REQUIRE(s.ref_peak == (float)(sp * sp) && s.hw == d.strehl_halfwin && s.npsf == d.npsf);
  // the frame kernel's tables
  REQUIRE(s.fused_ok == w.fused && s.otf_ok == w.otf);
  static const char *const frame_tabs[] = {"tile_info", "lit_info", "lit_count", "pair_info", "pair_count", "stripe_order", "psf_tw_h", "psf_tw_f",
                                           "qf_tab", "tile_mask", "tt_pk"};
  for (const char *t : frame_tabs) REQUIRE(has_tab(o, t) == (s.fused_ok != 0));
  if (!s.fused_ok) { REQUIRE(s.ntiles == 0 && s.otf_ok == 0); return; }
  const int nt = pd / 16;
  REQUIRE(s.ntiles == nt && pd % 16 == 0);
  const uint16_t *mask = tab<uint16_t>(o, "tile_mask", (size_t)pd * nt);
  for (int y = 0; y < pd; y++)
    for (int t = 0; t < nt; t++)
      for (int b = 0; b < 16; b++) REQUIRE(((mask[(size_t)y * nt + t] >> b) & 1) == (d.spupil[(size_t)y * pd + 16 * t + b] != 0.f));
  const int32_t *tinfo = tab<int32_t>(o, "tile_info", (size_t)nt * nt);
  int kinds[4] = {0, 0, 0, 0};           // unlit, partly lit without / with a sub-aperture, fully lit
  for (int r = 0; r < nt; r++)
    for (int t = 0; t < nt; t++) {
      int lit = 0, sub = -1;
      for (int yy = 0; yy < 16; yy++)
        for (int xx = 0; xx < 16; xx++) lit += d.spupil[(size_t)(16 * r + yy) * pd + 16 * t + xx] != 0.f;
      for (int i = 0; i < nv; i++)
        if (d.phasemap[i] == (pad + 16 * r) * n + pad + 16 * t) { REQUIRE(sub == -1); sub = i; }
      const int32_t want = (sub >= 0 ? sub | 0x40000 : 0) | ((lit || sub >= 0) ? 0x10000 : 0) | (lit == 256 ? 0x20000 : 0);
      REQUIRE(tinfo[r * nt + t] == want);
      kinds[lit == 0 ? 0 : lit == 256 ? 3 : sub >= 0 ? 2 : 1]++;
    }
  if (S.d.pupdiam == 64 && S.spupil[0] == 0.f) REQUIRE(kinds[0] && kinds[1] && kinds[2] && kinds[3]);      // the disc
  const int32_t *linfo = tab<int32_t>(o, "lit_info", (size_t)nt * (nt + 8)), *lcount = tab<int32_t>(o, "lit_count", nt);
  const int npm = (nt + 1) / 2 + 2;
  const int32_t *pinfo = tab<int32_t>(o, "pair_info", (size_t)nt * npm * 2), *pcount = tab<int32_t>(o, "pair_count", nt);
  std::vector<int> work(nt, 0);
  for (int r = 0; r < nt; r++) {
    std::vector<int32_t> want;
    for (int t = 0; t < nt; t++)
      if (tinfo[r * nt + t] & 0x10000) { want.push_back(tinfo[r * nt + t] | (t << 24)); work[r] += (tinfo[r * nt + t] & 0x40000) ? 4 : 1; }
    REQUIRE(lcount[r] == (int)want.size());
    for (int k = 0; k < nt + 8; k++)
      REQUIRE(linfo[(size_t)r * (nt + 8) + k] == (want.empty() ? 0 : want[std::min(k, (int)want.size() - 1)]));
    std::vector<int32_t> pw;
    for (int g = 0; 2 * g < nt; g++) {
      const int ta = 2 * g, tb = std::min(2 * g + 1, nt - 1);
      const bool la = (tinfo[r * nt + ta] & 0x10000) != 0, lb = 2 * g + 1 < nt && (tinfo[r * nt + tb] & 0x10000) != 0;
      if (!la && !lb) continue;
      pw.push_back((la ? tinfo[r * nt + ta] : 0) | (ta << 24));
      pw.push_back((lb ? tinfo[r * nt + tb] : 0) | (tb << 24));
    }
    REQUIRE(pcount[r] == (int)pw.size() / 2);
    for (int k = 0; k < npm; k++)
      for (int h = 0; h < 2; h++)
        REQUIRE(pinfo[((size_t)r * npm + k) * 2 + h] == (pw.empty() ? 0 : pw[2 * std::min(k, (int)pw.size() / 2 - 1) + h]));
  }
  const int32_t *order = tab<int32_t>(o, "stripe_order", nt);
  std::vector<int> used(nt, 0);
  for (int i = 0; i < nt; i++) {
    REQUIRE(order[i] >= 0 && order[i] < nt && !used[order[i]]++);
    if (i) REQUIRE(work[order[i - 1]] > work[order[i]] || (work[order[i - 1]] == work[order[i]] && order[i - 1] < order[i]));
  }
  // PSF operand against cos / sin in double; the split form adds up to the fp32 one
  const float *twf = tab<float>(o, "psf_tw_f", (size_t)nt * 64 * 4);
  const uint16_t *twh = tab<uint16_t>(o, "psf_tw_h", (size_t)nt * 64 * 8);
  for (int t = 0; t < nt; t++)
    for (int lane = 0; lane < 64; lane++)
      for (int j = 0; j < 4; j++) {
        const int x = 16 * t + 4 * (lane >> 4) + j, cc = lane & 15, k = cc < 8 ? cc + 1 : cc - 7;
        const double th = 2.0 * M_PI * (double)k * (double)x / (double)d.npsf;
        const float v = twf[((size_t)t * 64 + lane) * 4 + j];
        REQUIRE(fabs((double)v - (cc < 8 ? cos(th) : sin(th))) <= 1.2e-7);
        const uint16_t *h = &twh[((size_t)t * 64 + lane) * 8];
        REQUIRE(fabs((double)h2f(h[j]) + (double)h2f(h[4 + j]) - (double)v) <= ldexp(1.0, -21));
      }
  tab<float>(o, "qf_tab", 64 * 8);
  // tip-tilt planes at the target offsets
  const aomarl_dm_desc &T = d.dms[1];
  const float *tp = tab<float>(o, "tt_pk", (size_t)pd * pd * 2);
  for (int y = 0; y < pd; y++)
    for (int x = 0; x < pd; x++)
      for (int a = 0; a < 2; a++)
        REQUIRE(tp[((size_t)y * (pd / 4) + x / 4) * 8 + 4 * a + x % 4] == T.influ[2 * ((size_t)(y + (int)T.tar_yoff) * T.dim + (int)T.tar_xoff + x) + a]);
  // on-the-fly lattice: the nodes [g0, g0 + 4 nb) of a tile cover every actuator whose patch reaches it
  if (s.otf_ok) {
    const DevDm &Z = s.dms[0];
    REQUIRE(Z.sep && 16 % Z.pitch == 0 && s.otf_tpn == 16 / Z.pitch && s.otf_nb >= 1 && s.otf_nb <= 2 && s.otf_latw == (nt - 1) * s.otf_tpn + 4 * s.otf_nb);
    for (int axis = 0; axis < 2; axis++)
      for (int t = 0; t < nt; t++) {
        const int p0 = (axis ? Z.toy : Z.tox) + 16 * t, g0 = (axis ? s.otf_gy0 : s.otf_gx0) + t * s.otf_tpn, gmin = axis ? Z.j1min : Z.i1min;
        for (int g = 0; g < (axis ? Z.gh : Z.gw); g++) {
          const int X = gmin + Z.pitch * g;                       // the patch covers [X, X + ss)
          if (X < p0 + 16 && X + Z.ss > p0) REQUIRE(g >= g0 && g < g0 + 4 * s.otf_nb);
        }
        if (t == 0) REQUIRE((axis ? s.otf_yoff : s.otf_xoff) == p0 - (gmin + Z.pitch * g0));
      }
  }
}

// ---- the cases
static int g_cases = 0;
static bool g_table = false;
#ifdef CREATE_OUTCOME_EXTERN
static const bool g_new_too = false;       // the cases the replaced function cannot answer are left out
#else
static const bool g_new_too = true;
#endif

static void accepted(const char *name, const Geo &g, const Want &w) {
  g_case = name;
  Sys S;
  build(g, S);
  const Outcome o = outcome(&S.d);
  if (g_table) print_outcome(name, o);
  if (!o.ok) fprintf(stderr, "[%s] refused: %s\n", name, o.msg.c_str());
  REQUIRE(o.ok);
  check_accepted(S, o, w);
  g_cases++;
}
template <typename Fn>
static void refused(const char *name, const char *msg, Fn breakit, Geo g = Geo()) {
  g_case = name;
  Sys S;
  build(g, S);
  breakit(S);
  const Outcome o = outcome(&S.d);
  if (g_table) print_outcome(name, o);
  REQUIRE(!o.ok);
  if (o.msg != msg) fprintf(stderr, "[%s] message: %s\n", name, o.msg.c_str());
  REQUIRE(o.msg == msg);
  g_cases++;
}

static void accepted_cases() {
  Geo g;
  accepted("one_layer_pd32_pad0", g, Want{1, 1, 1, 1, 1});
  g = Geo(); g.pd = 64; g.pad = 8; g.pupil = DISC; g.nlayers = 3; g.dim[2] = 260; g.ns[2] = 24;
  accepted("three_layers_pd64_pad8_disc_shared_ab_big_screen", g, Want{1, 1, 1, 0, 1});
  g = Geo(); g.pd = 48; g.pad = 4; g.nlayers = 3; g.share[1] = 2;
  accepted("three_layers_pd48_odd_tiles", g, Want{1, 1, 1, 1, 1});
  g = Geo(); g.nlayers = 2;
  accepted("two_layers", g, Want{0, 0, 1, 1, 1});
  g = Geo(); g.hw = 4;
  accepted("halfwin_4", g, Want{0, 0, 1, 1, 1});
  g = Geo(); g.pupil = GREY;
  accepted("grey_pupil", g, Want{0, 0, 1, 1, 1});
  g = Geo(); g.pad = 4; g.tdx[0] = 1;
  accepted("window_offset_off_by_one", g, Want{0, 0, 1, 1, 1});
  g = Geo(); g.nlayers = 3; g.wox[1] = 4.5f; g.wox[2] = -3.f;
  accepted("fractional_offset_skips_window_tests", g, Want{0, 0, 1, 1, 0});
  g = Geo(); g.dm = DM_P12;
  accepted("dm_pitch_12", g, Want{1, 0, 1, 1, 1});
  g = Geo(); g.dm = DM_DIFFER;
  accepted("dm_patches_differ", g, Want{1, 0, 0, 1, 1});
  g = Geo(); g.dm = DM_DOUBLE;
  accepted("dm_two_actuators_one_cell", g, Want{1, 0, 0, 1, 1});
  g = Geo(); g.dm = DM_FINE;
  accepted("dm_pitch_too_fine", g, Want{1, 0, 0, 1, 1});
  g = Geo(); g.tt_first = true;
  accepted("tip_tilt_first", g, Want{0, 0, 1, 1, 1});
}

static const char *const kSampling = "unsupported WFS sampling (pdiam=%d nfft=%d nrebin=%d npix=%d, binmap, halfxy): the "
                                     "spot kernel is specialised for 16/64/2/16 with the standard half-pixel ramp";
static std::string sampling(int pdiam, int nfft, int nrebin, int npix) {
  char b[512];
  snprintf(b, sizeof(b), kSampling, pdiam, nfft, nrebin, npix);
  return b;
}

// one descriptor per refusal the replaced function had ("create: quadratic-form constants" cannot be provoked from a
// descriptor), in its order of tests
static void refused_cases() {
  {
    g_case = "null_descriptor";
    const Outcome o = outcome(nullptr);
    if (g_table) print_outcome(g_case, o);
    REQUIRE(!o.ok && o.msg == "aomarl_create: null argument");
    g_cases++;
  }
  refused("abi_version", "aomarl_create: ABI version 4, library is 5", [](Sys &S) { S.d.abi_version = 4; });
  refused("nlayers_9", "nlayers out of range", [](Sys &S) { S.d.nlayers = 9; });
  refused("ndm_0", "ndm out of range", [](Sys &S) { S.d.ndm = 0; });
  refused("n_below_pupdiam", "bad pupil sizes", [](Sys &S) { S.d.n = 28; });
  refused("pupdiam_34", "pupil grid sizes must be multiples of 4", [](Sys &S) { S.d.pupdiam = 34; S.d.n = 36; });
  refused("npsf_100", "npsf must be a power of two", [](Sys &S) { S.d.npsf = 100; });
  refused("halfwin_5", "strehl_halfwin must be 4, 8 or 16", [](Sys &S) { S.d.strehl_halfwin = 5; });
  refused("null_mpupil", "null host array in descriptor", [](Sys &S) { S.d.mpupil = nullptr; });
  refused("null_flux", "null host array in descriptor", [](Sys &S) { S.d.flux = nullptr; });
  refused("phasemap_outside", "phasemap tile outside the phase grid", [](Sys &S) { S.phasemap[1] = 20; });
  refused("phasemap_not_a_tile", "phasemap of sub-aperture 2 is not a contiguous tile", [](Sys &S) { S.phasemap[(size_t)17 * S.d.nvalid + 2]++; });
  refused("sampling_nfft_32", sampling(16, 32, 2, 16).c_str(), [](Sys &S) { S.d.nfft = 32; });
  refused("sampling_binmap", sampling(16, 64, 2, 16).c_str(), [](Sys &S) { S.binmap[256 + 9] += 2; });
  refused("sampling_halfxy", sampling(16, 64, 2, 16).c_str(), [](Sys &S) { S.halfxy[40] += 1e-4f; });
  refused("sampling_nfft_0", sampling(16, 0, 2, 16).c_str(), [](Sys &S) { S.d.nfft = 0; });
  refused("sampling_npix_0", sampling(16, 64, 2, 0).c_str(), [](Sys &S) { S.d.npix = 0; });
  refused("sampling_nrebin_0", sampling(16, 64, 0, 16).c_str(), [](Sys &S) { S.d.nrebin = 0; });
  refused("layer_dim_0", "bad layer 0", [](Sys &S) { S.d.layers[0].dim = 0; });
  refused("layer_narrower_than_ring", "layer 0: a screen of 40 pixels is narrower than the ring's 56 mirror columns", [](Sys &S) { S.d.layers[0].dim = 40; });
  refused("stencil_out_of_range", "stencil index out of range", [](Sys &S) { S.isty[0][3] = 96 * 96; });
  refused("wfs_window_leaves_screen", "WFS window leaves screen 0", [](Sys &S) { S.d.layers[0].wfs_xoff = 65; });
  refused("target_window_leaves_screen", "target window leaves screen 0", [](Sys &S) { S.d.layers[0].tar_yoff = -1; });
  refused("dm_influstart", "DM 0: influstart/ninflu inconsistent", [](Sys &S) { S.influstart[100]++; });
  refused("dm_ninflupos", "DM 0: sum(ninflu) != len(influpos)", [](Sys &S) { S.d.dms[0].ninflupos++; });
  refused("dm_influpos", "DM 0: influpos out of range", [](Sys &S) { S.influpos[50] = S.d.dms[0].nact * 32 * 32; });
  refused("tt_3_actuators", "tip-tilt DM must have 2 actuators", [](Sys &S) { S.d.dms[1].nact = 3; });
  refused("dm_type_7", "DM 1: unknown type 7", [](Sys &S) { S.d.dms[1].type = 7; });
  refused("wfs_window_leaves_dm", "WFS window leaves DM 0", [](Sys &S) { S.d.dms[0].wfs_yoff = 17; });
  refused("target_window_leaves_dm", "target window leaves DM 1", [](Sys &S) { S.d.dms[1].tar_xoff = -2; });
  refused("nactu", "sum of DM actuators (18) != nactu (17)", [](Sys &S) { S.d.nactu--; });
  refused("nslope", "nslope must be 2*nvalid", [](Sys &S) { S.d.nslope++; });
  refused("delay_3", "delay must be in [0, 2]", [](Sys &S) { S.d.delay = 3.f; });
  {
    // 128 tiles across: no sub-aperture, one layer of zeros
    Geo g;
    g.pd = 2048; g.dim[0] = 2064; g.ns[0] = 8; g.max_side = 4;
    refused("pupil_too_wide", "pupil too wide for the frame kernel's tile list", [](Sys &S) {
      S.d.nvalid = 0; S.d.nslope = 0; }, g);
  }
  if (!g_new_too) return;
  // the refusals that were host crashes
  if (g_table) printf("# from here on: the inputs that crashed the function the plan replaced; recorded from the plan itself\n");
  refused("null_halfxy", "null host array in descriptor", [](Sys &S) { S.d.halfxy = nullptr; });
  refused("null_istx", "null host array in descriptor", [](Sys &S) { S.d.layers[0].istx = nullptr; });
  refused("null_isty", "null host array in descriptor", [](Sys &S) { S.d.layers[0].isty = nullptr; });
  refused("null_A", "null host array in descriptor", [](Sys &S) { S.d.layers[0].A = nullptr; });
  refused("null_B", "null host array in descriptor", [](Sys &S) { S.d.layers[0].B = nullptr; });
  refused("nvalid_negative", "nvalid must not be negative", [](Sys &S) { S.d.nvalid = -1; });
  refused("sampling_pdiam_0", sampling(0, 64, 2, 16).c_str(), [](Sys &S) { S.d.pdiam = 0; });
  refused("npsf_0", "npsf must be a power of two", [](Sys &S) { S.d.npsf = 0; });
  refused("dm_dim_0", "DM 0: dim, nact and influsize must be positive", [](Sys &S) { S.d.dms[0].dim = 0; });
  refused("dm_influsize_0", "DM 0: dim, nact and influsize must be positive", [](Sys &S) { S.d.dms[0].influsize = 0; });
  refused("dm_nact_0", "DM 0: dim, nact and influsize must be positive", [](Sys &S) { S.d.dms[0].nact = 0; });
  refused("tt_dim_0", "DM 1: dim, nact and influsize must be positive", [](Sys &S) { S.d.dms[1].dim = 0; });
}

int main(int argc, char **argv) {
  g_table = argc > 1 && strcmp(argv[1], "--table") == 0;
  accepted_cases();
  refused_cases();
  printf("create_plan_host_check: ok (%d cases)\n", g_cases);
  return 0;
}
