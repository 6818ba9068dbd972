// aomarl_create_plan_host.h -- everything aomarl_create (aomarl_capi.hip) derives from an aomarl_desc before it touches
// the device: the refusals, the DevSys the kernels take, every table they walk, the host values the context keeps.  No
// HIP include, no global and no aomarl_ctx: the stand-alone host program (create_plan_host_check.cpp) runs the same text
// over descriptors of its own under the address and undefined-behaviour sanitizers, and tests/golden/create_plans.txt
// pins what it decides.  A wrong table here is a fault on the device, so this is where it has to be caught.
//
// create_plan() gives one of two things:
//   a refusal   false, and the message in CreatePlan::msg; nothing was allocated and no HIP call made.  Tests run in a
//               fixed order and the first one that fails wins; a table's null test sits where its upload used to.
//   a plan      sys       the DevSys with every scalar final and every pointer null
//               tables    what to upload, in order: name, bytes, and the place(s) in DevSys its device pointer goes to
//                         (byte offsets; layers of one [A | B] class name the same table).  What passes through unchanged
//                         refers to the descriptor's memory (ref), so creation makes no extra pass over the large arrays;
//                         what is derived is owned by the plan
//               host      the values the context keeps for scheduling and for the geometric controller
//               production_layout   two mirrors, a stack array then a tip-tilt, and one or three layers: the layout the
//                         specialised spot, target and frame kernels are instantiated for (the ONE place that says so)
// Two things stay with the executor: the [hi | lo] split-fp16 form of the PSF operand (no _Float16 in host C++ here: the
// plan carries the fp32 form, tables[psf_operand]) and the power-of-two scales of the [A | B] tables (gemm_scale, on
// tables[ab_table[cls]]).
#pragma once
#include "aomarl_sys.h"
#include "aomarl_move_plan_host.h"     // MOVE_SMALL_DIM, MOVE_SMALL_K
#include "aomarl_qf4_host.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

// k_dm_shape_sep: pixels of a block's tile, and the lattice cells that can reach it (staged in LDS)
constexpr int DMS_TX = 64, DMS_TY = 32, DMS_GX = 9, DMS_GY = 8;

struct CreateTable {
  std::string name;                    // the DevSys field it goes to (the first one, if several)
  const void *ref = nullptr;           // the descriptor's memory, or null: own
  std::vector<unsigned char> own;
  size_t bytes = 0;
  std::vector<size_t> slots;           // byte offsets into DevSys
  const void *data() const { return ref ? ref : (const void *)own.data(); }
};

struct CreateHost {
  int dim[AOMARL_MAX_LAYERS], ns[AOMARL_MAX_LAYERS], abclass[AOMARL_MAX_LAYERS];
  float deltax[AOMARL_MAX_LAYERS], deltay[AOMARL_MAX_LAYERS];
  int nclass = 0;
  int maxdim = 0, maxK = 0;
  bool small_ok = false;               // every layer has dim <= MOVE_SMALL_DIM, ns + dim <= MOVE_SMALL_K (transposed [A|B] in the tables)
  float gain = 0.f, delay = 0.f;
  std::vector<int32_t> h_grid;         // [gh][gw] actuator index or -1 (stack-array DM 0)
  std::vector<float> h_prof, h_spupil, h_tt;
};

struct CreatePlan {
  char msg[512] = "";
  DevSys sys;
  std::vector<CreateTable> tables;
  CreateHost host;
  bool production_layout = false;
  int ab_table[AOMARL_MAX_LAYERS];     // [nclass] index of the class's [A | B] in tables
  int psf_operand = -1;                // index of psf_tw_f in tables, or -1 (no frame kernel)
};

static inline bool create_refuse(CreatePlan &P, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(P.msg, sizeof(P.msg), fmt, ap);
  va_end(ap);
  return false;
}

// One table of n elements for the pointer at `slot` (a field of P.sys).  As the upload it describes: nothing for
// n == 0 (the pointer stays null), a null array is refused.  copy: the plan owns the bytes (host is a temporary).
template <typename T>
static inline bool create_table(CreatePlan &P, const std::string &name, const T *host, size_t n, bool copy, const void *slot,
                                int *index = nullptr) {
  if (index) *index = -1;
  if (n == 0) return true;
  if (!host) return create_refuse(P, "null host array in descriptor");
  P.tables.emplace_back();
  CreateTable &t = P.tables.back();
  t.name = name; t.bytes = n * sizeof(T);
  if (copy) t.own.assign((const unsigned char *)host, (const unsigned char *)host + t.bytes);
  else t.ref = host;
  t.slots.push_back((size_t)((const char *)slot - (const char *)&P.sys));
  if (index) *index = (int)P.tables.size() - 1;
  return true;
}
static inline void create_also(CreatePlan &P, int index, const void *slot) {
  if (index >= 0) P.tables[index].slots.push_back((size_t)((const char *)slot - (const char *)&P.sys));
}
static inline std::string create_name(const char *fmt, int i) {
  char b[64];
  snprintf(b, sizeof(b), fmt, i);
  return b;
}

#define CP_TRY(x) do { if (!(x)) return false; } while (0)
#define CP_REF(T, host, n, dev) CP_TRY(create_table<T>(P, #dev, host, n, false, &s.dev))
#define CP_OWN(T, host, n, dev) CP_TRY(create_table<T>(P, #dev, host, n, true, &s.dev))

static inline bool create_is_int(float v) { return floorf(v) == v; }

static inline bool create_refuse_sampling(CreatePlan &P, const aomarl_desc *d) {
  return create_refuse(P, "unsupported WFS sampling (pdiam=%d nfft=%d nrebin=%d npix=%d, binmap, halfxy): the "
                          "spot kernel is specialised for 16/64/2/16 with the standard half-pixel ramp",
                       d->pdiam, d->nfft, d->nrebin, d->npix);
}

// ---- WFS sampling: the sub-aperture tiles recovered from phasemap (sub: x0 | y0 << 16 of each), the binning map and
// the half-pixel ramp the spot kernel hard-codes
static inline bool create_plan_wfs(const aomarl_desc *d, CreatePlan &P, std::vector<int32_t> &sub) {
  DevSys &s = P.sys;
  s.nvalid = d->nvalid; s.pdiam = d->pdiam; s.nfft = d->nfft; s.npix = d->npix;
  s.nrebin = d->nrebin; s.nxsub = d->nxsub;
  if (d->nvalid < 0) return create_refuse(P, "nvalid must not be negative");
  if (d->pdiam <= 0 || d->nfft <= 0 || d->npix <= 0 || d->nrebin <= 0) return create_refuse_sampling(P, d);
  const int pd2 = d->pdiam * d->pdiam;
  CP_REF(int32_t, d->phasemap, (size_t)pd2 * d->nvalid, phasemap);
  // every sub-aperture must be a contiguous pdiam x pdiam tile of the phase grid
  sub.assign(d->nvalid, 0);
  for (int i = 0; i < d->nvalid; i++) {
    int p0 = d->phasemap[i];
    int x0 = p0 % d->n, y0 = p0 / d->n;
    if (x0 + d->pdiam > d->n || y0 + d->pdiam > d->n) return create_refuse(P, "phasemap tile outside the phase grid");
    for (int k = 0; k < pd2; k++)
      if (d->phasemap[(size_t)k * d->nvalid + i] != p0 + (k % d->pdiam) + d->n * (k / d->pdiam))
        return create_refuse(P, "phasemap of sub-aperture %d is not a contiguous tile", i);
    sub[i] = x0 | (y0 << 16);
  }
  CP_OWN(int32_t, sub.data(), sub.size(), sub_xy);
  if (!d->halfxy) return create_refuse(P, "null host array in descriptor");
  std::vector<float> hrev(pd2);
  for (int k = 0; k < pd2; k++) hrev[k] = (float)((double)d->halfxy[k] / (2.0 * M_PI));
  CP_OWN(float, hrev.data(), hrev.size(), halfxy);
  CP_REF(int32_t, d->binmap, (size_t)d->nrebin * d->nrebin * d->npix * d->npix, binmap);
  CP_REF(float, d->flux, (size_t)d->nvalid, flux);
  CP_TRY(create_table<int32_t>(P, "validx", d->validsubsx, (size_t)d->nvalid, false, &s.validx));
  CP_TRY(create_table<int32_t>(P, "validy", d->validsubsy, (size_t)d->nvalid, false, &s.validy));
  s.nphot = d->nphot; s.wfs_inv_lambda = 1.0f / d->wfs_lambda; s.noise = d->noise;
  s.cog_offset = d->cog_offset; s.cog_scale = d->cog_scale; s.subapd = d->subapd;
  bool spot_fast = (d->pdiam == 16 && d->nfft == 64 && d->nrebin == 2 && d->npix == 16);
  if (spot_fast) {
    // the kernel hard-codes the binmap of this sampling: LR (Y, X) <- HR rows/cols
    // (2Y-16 .. 2Y-15) mod 64 ; check the map handed in says the same
    for (int px = 0; px < 256 && spot_fast; px++) {
      int Y = px / 16, X = px % 16;
      bool seen[4] = {false, false, false, false};
      for (int r = 0; r < 4; r++) {
        int hr = d->binmap[r * 256 + px];
        int ky = hr / 64, kx = hr % 64;
        int dy = (ky - (2 * Y - 16) + 64) % 64, dx = (kx - (2 * X - 16) + 64) % 64;
        if (dy > 1 || dx > 1) { spot_fast = false; break; }
        seen[dy * 2 + dx] = true;
      }
      if (!(seen[0] && seen[1] && seen[2] && seen[3])) spot_fast = false;
    }
  }
  if (spot_fast) {
    // the kernel folds the half-pixel ramp into half-integer DFT frequencies: it must be the
    // reference's halfxy = pi (x + y) / Nfft (geom_init.py:689-692)
    for (int k = 0; k < pd2 && spot_fast; k++) {
      double want = M_PI * (double)((k % d->pdiam) + (k / d->pdiam)) / (double)d->nfft;
      if (fabs((double)d->halfxy[k] - want) > 2e-6) spot_fast = false;
    }
  }
  if (!spot_fast) return create_refuse_sampling(P, d);
  return true;
}

// ---- layers: packed stencils, [A | B] per sharing class (and its transpose for the small screens), the windows
static inline bool create_plan_layers(const aomarl_desc *d, CreatePlan &P) {
  DevSys &s = P.sys;
  CreateHost &H = P.host;
  s.nlayers = d->nlayers;
  long long off = 0;
  const float *seenA[AOMARL_MAX_LAYERS]; const float *seenB[AOMARL_MAX_LAYERS];
  int tabAB[AOMARL_MAX_LAYERS]; int ldab[AOMARL_MAX_LAYERS];
  int tabABt[AOMARL_MAX_LAYERS]; int ldt[AOMARL_MAX_LAYERS];
  H.small_ok = true;
  s.wfs_all_int = 1; s.tar_all_int = 1;
  for (int l = 0; l < d->nlayers; l++) {
    const aomarl_layer_desc &L = d->layers[l];
    DevLayer &D = s.layers[l];
    if (L.dim <= 0 || L.dim > 65535 || L.nstencil <= 0) return create_refuse(P, "bad layer %d", l);
    // the mirror columns repeat the row's first RING_PAD pixels: a narrower screen would mirror pixels it is
    // writing (k_refresh_mirror, k_set_screen, the scatter's px < RING_PAD)
    if (L.dim < RING_PAD) return create_refuse(P, "layer %d: a screen of %d pixels is narrower than the ring's %d mirror columns", l, L.dim, RING_PAD);
    D.dim = L.dim; D.ns = L.nstencil; D.screen_off = off; off += (long long)L.dim * (L.dim + RING_PAD);
    H.dim[l] = L.dim; H.ns[l] = L.nstencil; H.deltax[l] = L.deltax; H.deltay[l] = L.deltay;
    if (L.dim > H.maxdim) H.maxdim = L.dim;
    if (L.dim + L.nstencil > H.maxK) H.maxK = L.dim + L.nstencil;
    if (!L.istx || !L.isty) return create_refuse(P, "null host array in descriptor");
    std::vector<uint32_t> ix(L.nstencil), iy(L.nstencil);
    for (int k = 0; k < L.nstencil; k++) {
      if (L.istx[k] >= (uint32_t)(L.dim * L.dim) || L.isty[k] >= (uint32_t)(L.dim * L.dim)) return create_refuse(P, "stencil index out of range");
      ix[k] = (L.istx[k] % L.dim) | ((L.istx[k] / L.dim) << 16);
      iy[k] = (L.isty[k] % L.dim) | ((L.isty[k] / L.dim) << 16);
    }
    CP_TRY(create_table<uint32_t>(P, create_name("layers[%d].istx", l), ix.data(), ix.size(), true, &D.istx));
    CP_TRY(create_table<uint32_t>(P, create_name("layers[%d].isty", l), iy.data(), iy.size(), true, &D.isty));
    {
      std::vector<uint32_t> it(ix.size());
      for (size_t k = 0; k < ix.size(); k++) it[k] = (ix[k] >> 16) | (ix[k] << 16);
      CP_TRY(create_table<uint32_t>(P, create_name("layers[%d].istT", l), it.data(), it.size(), true, &D.istT));
    }
    // [A | B] concatenated, shared between layers that were given the same host matrices
    int cls = -1;
    for (int m = 0; m < H.nclass; m++)
      if (seenA[m] == L.A && seenB[m] == L.B) cls = m;
    if (cls < 0) {
      if (!L.A || !L.B) return create_refuse(P, "null host array in descriptor");
      cls = H.nclass++;
      seenA[cls] = L.A; seenB[cls] = L.B;
      int K = L.nstencil + L.dim;
      int ld = (K + 3) & ~3;
      std::vector<float> ab((size_t)L.dim * ld, 0.f);
      for (int r = 0; r < L.dim; r++) {
        memcpy(&ab[(size_t)r * ld], L.A + (size_t)r * L.nstencil, sizeof(float) * L.nstencil);
        memcpy(&ab[(size_t)r * ld + L.nstencil], L.B + (size_t)r * L.dim, sizeof(float) * L.dim);
      }
      CP_TRY(create_table<float>(P, create_name("layers[%d].AB", l), ab.data(), ab.size(), true, &D.AB, &tabAB[cls]));
      ldab[cls] = ld;
      tabABt[cls] = -1; ldt[cls] = 0;
      if (L.dim <= MOVE_SMALL_DIM && K <= MOVE_SMALL_K) {          // small screens: the transpose for k_move_small
        const int lt = (L.dim + 63) & ~63;
        std::vector<float> abt((size_t)K * lt, 0.f);
        for (int r = 0; r < L.dim; r++)
          for (int j = 0; j < K; j++) abt[(size_t)j * lt + r] = ab[(size_t)r * ld + j];
        CP_TRY(create_table<float>(P, create_name("layers[%d].ABt", l), abt.data(), abt.size(), true, &D.ABt, &tabABt[cls]));
        ldt[cls] = lt;
      }
      P.ab_table[cls] = tabAB[cls];
    } else {
      create_also(P, tabAB[cls], &D.AB);
      create_also(P, tabABt[cls], &D.ABt);
    }
    H.abclass[l] = cls;
    D.ldab = ldab[cls];
    D.ldt = ldt[cls];
    if (tabABt[cls] < 0) H.small_ok = false;
    D.amp = L.amplitude;
    D.wxo = L.wfs_xoff; D.wyo = L.wfs_yoff; D.txo = L.tar_xoff; D.tyo = L.tar_yoff;
    D.wox = (int)L.wfs_xoff; D.woy = (int)L.wfs_yoff; D.tox = (int)L.tar_xoff; D.toy = (int)L.tar_yoff;
    if (!create_is_int(L.wfs_xoff) || !create_is_int(L.wfs_yoff)) s.wfs_all_int = 0;
    if (!create_is_int(L.tar_xoff) || !create_is_int(L.tar_yoff)) s.tar_all_int = 0;
    if (s.wfs_all_int && (D.wox < 0 || D.woy < 0 || D.wox + d->n > L.dim || D.woy + d->n > L.dim)) return create_refuse(P, "WFS window leaves screen %d", l);
    if (s.tar_all_int && (D.tox < 0 || D.toy < 0 || D.tox + d->pupdiam > L.dim || D.toy + d->pupdiam > L.dim)) return create_refuse(P, "target window leaves screen %d", l);
  }
  s.screen_stride = off;
  return true;
}

// ---- separable-lattice fast path of a stack-array mirror: recover (i1, j1) of every actuator from the gather
// tables (first pixel that references sample 0 of its patch), check that all patches are
// one rank-1 profile and that the actuators sit on a regular lattice.  false: the generic gather tables.
static inline bool create_dm_lattice(const aomarl_dm_desc &M, DevDm &D, std::vector<int32_t> &grid, std::vector<float> &prof) {
  const int ss = M.influsize, ss2 = ss * ss, na = M.nact;
  std::vector<int> i1(na, INT32_MIN), j1(na, INT32_MIN);
  for (long long p = 0; p < (long long)M.dim * M.dim; p++)
    for (int t = 0; t < M.ninflu[p]; t++) {
      int pos = M.influpos[M.influstart[p] + t];
      int act = pos / ss2, rem = pos % ss2, a = rem / ss, b = rem % ss;   // b: x offset
      int x = (int)(p % M.dim) - b, y = (int)(p / M.dim) - a;
      if (i1[act] == INT32_MIN) { i1[act] = x; j1[act] = y; }
      else if (i1[act] != x || j1[act] != y) { i1[act] = INT32_MAX; }
    }
  bool ok = na > 0 && ss <= 128;
  for (int a = 0; a < na && ok; a++) ok = (i1[a] != INT32_MIN && i1[a] != INT32_MAX);
  // identical patches
  for (int a = 1; a < na && ok; a++)
    ok = memcmp(M.influ + (size_t)a * ss2, M.influ, sizeof(float) * ss2) == 0;
  prof.assign(ss, 0.f);
  if (ok) {
    int cdx = 0; float best = 0.f;
    for (int t = 0; t < ss; t++) if (M.influ[t * ss + t] > best) { best = M.influ[t * ss + t]; cdx = t; }
    ok = best > 0.f;
    if (ok) {
      const float sc = 1.0f / sqrtf(best);
      float mx = 0.f;
      for (int t = 0; t < ss; t++) prof[t] = M.influ[t * ss + cdx] * sc;
      for (int a = 0; a < ss; a++)
        for (int b = 0; b < ss; b++) mx = fmaxf(mx, fabsf(M.influ[a * ss + b] - prof[a] * prof[b]));
      ok = mx <= 2e-6f * best;
    }
  }
  int pitch = 0, imin = INT32_MAX, jmin = INT32_MAX, imax = INT32_MIN, jmax = INT32_MIN;
  if (ok) {
    auto gcd = [](int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; };
    for (int a = 0; a < na; a++) { imin = std::min(imin, i1[a]); jmin = std::min(jmin, j1[a]); imax = std::max(imax, i1[a]); jmax = std::max(jmax, j1[a]); }
    for (int a = 0; a < na; a++) { pitch = gcd(pitch, i1[a] - imin); pitch = gcd(pitch, j1[a] - jmin); }
    ok = pitch > 0 && ss <= 4 * pitch && (DMS_TX + ss - 1) / pitch + 2 <= DMS_GX && (DMS_TY + ss - 1) / pitch + 2 <= DMS_GY;
  }
  if (ok) {
    const int gw = (imax - imin) / pitch + 1, gh = (jmax - jmin) / pitch + 1;
    grid.assign((size_t)gw * gh, -1);
    for (int a = 0; a < na && ok; a++) {
      int32_t &cell = grid[(size_t)((j1[a] - jmin) / pitch) * gw + (i1[a] - imin) / pitch];
      if (cell != -1) ok = false;
      cell = a;
    }
    if (ok) { D.sep = 1; D.pitch = pitch; D.i1min = imin; D.j1min = jmin; D.gw = gw; D.gh = gh; }
  }
  return ok;
}

// ---- one mirror: its gather tables checked (a bad table would fault on the device), the lattice, the windows
static inline bool create_plan_dm(const aomarl_desc *d, int k, CreatePlan &P, long long &soff, int &coff) {
  DevSys &s = P.sys;
  const aomarl_dm_desc &M = d->dms[k];
  DevDm &D = s.dms[k];
  D.type = M.type; D.dim = M.dim; D.nact = M.nact; D.ss = M.influsize;
  D.shape_off = soff;
  soff += (M.type == AOMARL_DM_TT) ? 4 : (long long)M.dim * M.dim;   // TT: 2 commands (+pad)
  D.com_off = coff; coff += M.nact;
  if (M.type == AOMARL_DM_PZT) {
    if (M.dim <= 0 || M.nact <= 0 || M.influsize <= 0) return create_refuse(P, "DM %d: dim, nact and influsize must be positive", k);
    CP_TRY(create_table<float>(P, create_name("dms[%d].influ", k), M.influ, (size_t)M.nact * M.influsize * M.influsize, false, &D.influ));
    CP_TRY(create_table<int32_t>(P, create_name("dms[%d].influpos", k), M.influpos, (size_t)M.ninflupos, false, &D.influpos));
    CP_TRY(create_table<int32_t>(P, create_name("dms[%d].ninflu", k), M.ninflu, (size_t)M.dim * M.dim, false, &D.ninflu));
    CP_TRY(create_table<int32_t>(P, create_name("dms[%d].influstart", k), M.influstart, (size_t)M.dim * M.dim, false, &D.influstart));
    // bounds of the gather tables
    long long tot = 0;
    for (long long p = 0; p < (long long)M.dim * M.dim; p++) {
      if (M.influstart[p] != tot || M.ninflu[p] < 0) return create_refuse(P, "DM %d: influstart/ninflu inconsistent", k);
      tot += M.ninflu[p];
    }
    if (tot != M.ninflupos) return create_refuse(P, "DM %d: sum(ninflu) != len(influpos)", k);
    for (long long q = 0; q < M.ninflupos; q++)
      if (M.influpos[q] < 0 || M.influpos[q] >= M.nact * M.influsize * M.influsize) return create_refuse(P, "DM %d: influpos out of range", k);
    std::vector<int32_t> grid;
    std::vector<float> prof;
    if (create_dm_lattice(M, D, grid, prof)) {
      CP_TRY(create_table<int32_t>(P, create_name("dms[%d].grid", k), grid.data(), grid.size(), true, &D.grid));
      CP_TRY(create_table<float>(P, create_name("dms[%d].prof", k), prof.data(), prof.size(), true, &D.prof));
      if (k == 0) { P.host.h_grid = grid; P.host.h_prof = prof; }
    }
  } else if (M.type == AOMARL_DM_TT) {
    if (M.nact != 2) return create_refuse(P, "tip-tilt DM must have 2 actuators");
    if (M.dim <= 0) return create_refuse(P, "DM %d: dim, nact and influsize must be positive", k);
    CP_TRY(create_table<float>(P, create_name("dms[%d].influ", k), M.influ, (size_t)M.dim * M.dim * 2, false, &D.influ));
    if (k == 1) P.host.h_tt.assign(M.influ, M.influ + (size_t)M.dim * M.dim * 2);
  } else {
    return create_refuse(P, "DM %d: unknown type %d", k, M.type);
  }
  D.wxo = M.wfs_xoff; D.wyo = M.wfs_yoff; D.txo = M.tar_xoff; D.tyo = M.tar_yoff;
  D.wox = (int)M.wfs_xoff; D.woy = (int)M.wfs_yoff; D.tox = (int)M.tar_xoff; D.toy = (int)M.tar_yoff;
  if (!create_is_int(M.wfs_xoff) || !create_is_int(M.wfs_yoff)) s.wfs_all_int = 0;
  if (!create_is_int(M.tar_xoff) || !create_is_int(M.tar_yoff)) s.tar_all_int = 0;
  if (s.wfs_all_int && (D.wox < 0 || D.woy < 0 || D.wox + d->n > M.dim || D.woy + d->n > M.dim)) return create_refuse(P, "WFS window leaves DM %d", k);
  if (s.tar_all_int && (D.tox < 0 || D.toy < 0 || D.tox + d->pupdiam > M.dim || D.toy + d->pupdiam > M.dim)) return create_refuse(P, "target window leaves DM %d", k);
  return true;
}

// ---- target: the PSF's twiddles, the reference peak
static inline bool create_plan_target(const aomarl_desc *d, CreatePlan &P) {
  DevSys &s = P.sys;
  s.tar_inv_lambda = 1.0f / d->tar_lambda; s.npsf = d->npsf; s.hw = d->strehl_halfwin;
  std::vector<float> tw((size_t)d->npsf * 2);
  for (int j = 0; j < d->npsf; j++) {
    double a = 2.0 * M_PI * (double)j / (double)d->npsf;
    tw[2 * j] = (float)cos(a); tw[2 * j + 1] = (float)sin(a);
  }
  CP_OWN(float, tw.data(), tw.size(), psf_tw);
  double sp = 0.;
  for (size_t p = 0; p < (size_t)d->pupdiam * d->pupdiam; p++) sp += d->spupil[p];
  s.ref_peak = (float)(sp * sp);
  return true;
}

// ---- frame tiles.  ok (in: the layout and the windows line up; out: the tiles do too -- binary pupil, one sub-aperture
// per tile at most, on the tile grid).  With ok: tile_info (and tmask for tile_mask), the lit tiles one by one and in
// pairs, the stripes by decreasing work
static inline bool create_plan_tiles(const aomarl_desc *d, CreatePlan &P, const std::vector<int32_t> &sub, bool &ok,
                                     std::vector<uint16_t> &tmask) {
  DevSys &s = P.sys;
  const int pd = d->pupdiam, pad = (d->n - pd) / 2;
  for (int y = 0; y < pd && ok; y++)
    for (int x = 0; x < pd && ok; x++) {
      const float m = d->spupil[(size_t)y * pd + x];
      ok = (m == 0.f || m == 1.f) && d->mpupil[(size_t)(y + pad) * d->n + x + pad] == m;
    }
  const int nt = pd / 16;
  std::vector<int32_t> tsub((size_t)std::max(nt * nt, 1), -1);
  tmask.assign((size_t)std::max(pd * nt, 1), 0);
  if (ok) {
    for (int y = 0; y < pd; y++)
      for (int x = 0; x < pd; x++)
        if (d->spupil[(size_t)y * pd + x] != 0.f) tmask[(size_t)y * nt + x / 16] |= (uint16_t)(1u << (x % 16));
    for (int r = 0; r < nt; r++)
      for (int t = 0; t < nt; t++) {
        bool lit = false;
        for (int yy = 0; yy < 16; yy++) lit = lit || tmask[(size_t)(16 * r + yy) * nt + t] != 0;
        if (!lit) tsub[(size_t)r * nt + t] = -2;
      }
    for (int i = 0; i < d->nvalid && ok; i++) {
      const int x0 = (sub[i] & 0xFFFF) - pad, y0 = (sub[i] >> 16) - pad;
      ok = x0 >= 0 && y0 >= 0 && x0 % 16 == 0 && y0 % 16 == 0 && x0 < pd && y0 < pd;
      if (ok) {
        int32_t &cell = tsub[(size_t)(y0 / 16) * nt + x0 / 16];
        ok = cell < 0;                 // one sub-aperture per tile (an unlit tile with a
        cell = i;                      // sub-aperture is still imaged: zero flux, zero slopes)
      }
    }
  }
  if (!ok) return true;
  // tile_info: [15:0] sub-aperture, bit 16 lit, 17 every pixel lit, 18 valid sub-aperture
  std::vector<int32_t> tinfo(tsub.size(), 0);
  for (int r = 0; r < nt; r++)
    for (int t = 0; t < nt; t++) {
      const int32_t sb = tsub[(size_t)r * nt + t];
      bool full = true;
      for (int yy = 0; yy < 16; yy++) full = full && tmask[(size_t)(16 * r + yy) * nt + t] == 0xFFFF;
      int32_t v = 0;
      if (sb != -2) v |= 0x10000;
      if (full) v |= 0x20000;
      if (sb >= 0) { v |= 0x40000 | sb; v |= 0x10000; }     // an unlit tile with a sub-aperture is still imaged
      tinfo[(size_t)r * nt + t] = v;
    }
  CP_OWN(int32_t, tinfo.data(), tinfo.size(), tile_info);
  {
    if (nt > 127) return create_refuse(P, "pupil too wide for the frame kernel's tile list");
    std::vector<int32_t> linfo((size_t)nt * (nt + 8), 0), lcount(nt, 0);
    for (int r = 0; r < nt; r++) {
      int k = 0;
      for (int t = 0; t < nt; t++)
        if (tinfo[(size_t)r * nt + t] & 0x10000) linfo[(size_t)r * (nt + 8) + k++] = tinfo[(size_t)r * nt + t] | (t << 24);
      lcount[r] = k;
      for (int kk = k; kk < nt + 8; kk++) linfo[(size_t)r * (nt + 8) + kk] = k ? linfo[(size_t)r * (nt + 8) + k - 1] : 0;
    }
    CP_OWN(int32_t, linfo.data(), linfo.size(), lit_info);
    CP_OWN(int32_t, lcount.data(), lcount.size(), lit_count);
    // the same tiles in pairs (2 g, 2 g + 1): the frame kernel fetches the layer rows of a pair as whole
    // 128-byte pieces
    const int npm = (nt + 1) / 2 + 2;
    std::vector<int32_t> pinfo((size_t)nt * npm * 2, 0), pcount(nt, 0);
    for (int r = 0; r < nt; r++) {
      int k = 0;
      int32_t *row = &pinfo[(size_t)r * npm * 2];
      for (int g = 0; 2 * g < nt; g++) {
        const int ta = 2 * g, tb = 2 * g + 1 < nt ? 2 * g + 1 : 2 * g;
        const int32_t va = tinfo[(size_t)r * nt + ta], vb = 2 * g + 1 < nt ? tinfo[(size_t)r * nt + tb] : 0;
        if (!((va | vb) & 0x10000)) continue;
        row[2 * k] = ((va & 0x10000) ? va : 0) | (ta << 24);
        row[2 * k + 1] = ((vb & 0x10000) ? vb : 0) | (tb << 24);
        k++;
      }
      pcount[r] = k;
      for (int kk = k; kk < npm; kk++) {
        row[2 * kk] = k ? row[2 * (k - 1)] : 0;
        row[2 * kk + 1] = k ? row[2 * (k - 1) + 1] : 0;
      }
    }
    CP_OWN(int32_t, pinfo.data(), pinfo.size(), pair_info);
    CP_OWN(int32_t, pcount.data(), pcount.size(), pair_count);
  }
  {
    std::vector<int32_t> order(nt), work(nt, 0);
    for (int r = 0; r < nt; r++) {
      order[r] = r;
      for (int t = 0; t < nt; t++) {
        const int32_t v = tinfo[(size_t)r * nt + t];
        work[r] += (v & 0x10000) ? ((v & 0x40000) ? 4 : 1) : 0;   // a sub-aperture tile costs ~4x a bare one
      }
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return work[a] > work[b]; });
    CP_OWN(int32_t, order.data(), order.size(), stripe_order);
  }
  return true;
}

// ---- PSF operand of the frame kernel for lane (q, c) of tile t: X = 16 t + 4 q + j (j = 0..3), column c of
// [cos 2 pi k X / npsf (k = 1..8) | sin 2 pi k X / npsf (k = 1..8)]; the fp32 form (the executor forms [hi | lo] from it)
static inline bool create_plan_psf_operand(const aomarl_desc *d, CreatePlan &P, int nt) {
  DevSys &s = P.sys;
  std::vector<float> twf((size_t)nt * 64 * 4);
  for (int t = 0; t < nt; t++)
    for (int lane = 0; lane < 64; lane++)
      for (int j = 0; j < 4; j++) {
        const int x = 16 * t + 4 * (lane >> 4) + j, cc = lane & 15;
        const int k = cc < 8 ? cc + 1 : cc - 7;
        const double th = 2.0 * M_PI * (double)(((long long)k * x) % d->npsf) / (double)d->npsf;
        const float v = (float)(cc < 8 ? cos(th) : sin(th));
        twf[((size_t)t * 64 + lane) * 4 + j] = v;
      }
  CP_TRY(create_table<float>(P, "psf_tw_f", twf.data(), twf.size(), true, &s.psf_tw_f, &P.psf_operand));
  return true;
}

// ---- tip-tilt planes as the frame kernel reads them (k_frame_wave: tvo): pupil pixel (y, 4 g + j)
static inline bool create_plan_tt_planes(const aomarl_desc *d, CreatePlan &P) {
  DevSys &s = P.sys;
  const int pd = d->pupdiam;
  const DevDm &T = s.dms[1];
  std::vector<float> tp((size_t)pd * pd * 2);
  for (int y = 0; y < pd; y++)
    for (int g = 0; g < pd / 4; g++)
      for (int j = 0; j < 4; j++) {
        const size_t o = (size_t)(y + T.toy) * T.dim + T.tox + 4 * g + j;
        float *dst = &tp[((size_t)y * (pd / 4) + g) * 8];
        dst[j] = P.host.h_tt[2 * o]; dst[4 + j] = P.host.h_tt[2 * o + 1];
      }
  CP_OWN(float, tp.data(), tp.size(), tt_pk);
  return true;
}

// ---- on-the-fly lattice: the stack-array DM evaluated from the command lattice inside the frame kernel
static inline void create_plan_otf(CreatePlan &P, int nt) {
  DevSys &s = P.sys;
  const DevDm &Z = s.dms[0];
  s.otf_ok = 0;
  if (Z.sep && Z.pitch > 0 && 16 % Z.pitch == 0) {
    auto first = [&](int p0, int pmin) {
      const int num = p0 - pmin - (Z.ss - 1);
      return num >= 0 ? (num + Z.pitch - 1) / Z.pitch : -((-num) / Z.pitch);
    };
    s.otf_gx0 = first(Z.tox, Z.i1min); s.otf_gy0 = first(Z.toy, Z.j1min);
    s.otf_xoff = Z.tox - (Z.i1min + Z.pitch * s.otf_gx0);
    s.otf_yoff = Z.toy - (Z.j1min + Z.pitch * s.otf_gy0);
    const int cnt = std::max((s.otf_xoff + 15) / Z.pitch + 1, (s.otf_yoff + 15) / Z.pitch + 1);
    s.otf_nb = (cnt + 3) / 4; s.otf_tpn = 16 / Z.pitch;
    s.otf_latw = (nt - 1) * s.otf_tpn + 4 * s.otf_nb;
    s.otf_ok = (s.otf_nb >= 1 && s.otf_nb <= 2 && s.otf_xoff >= 0 && s.otf_yoff >= 0) ? 1 : 0;
  }
}

// ---- fused frame kernel: the WFS tiles must BE the tiles of the pupil grid, at the same
// screen / DM pixels, the pupil must be binary
static inline bool create_plan_frame(const aomarl_desc *d, CreatePlan &P, const std::vector<int32_t> &sub) {
  DevSys &s = P.sys;
  s.fused_ok = 0; s.ntiles = 0;
  const int pd = d->pupdiam, pad = (d->n - pd) / 2;
  bool ok = s.wfs_all_int && s.tar_all_int && P.production_layout &&
            d->strehl_halfwin == 8 && pd % 16 == 0 && pad >= 0 && d->n == pd + 2 * pad && d->nvalid <= 0xFFFF &&
            (d->npsf & (d->npsf - 1)) == 0 && d->npsf <= 4096 && pd / 16 <= 256;
  for (int l = 0; l < d->nlayers && ok; l++)
    ok = s.layers[l].wox + pad == s.layers[l].tox && s.layers[l].woy + pad == s.layers[l].toy;
  for (int k = 0; k < d->ndm && ok; k++)
    ok = s.dms[k].wox + pad == s.dms[k].tox && s.dms[k].woy + pad == s.dms[k].toy;
  const int nt = pd / 16;
  std::vector<uint16_t> tmask;
  CP_TRY(create_plan_tiles(d, P, sub, ok, tmask));
  if (!ok) return true;
  CP_TRY(create_plan_psf_operand(d, P, nt));
  {
    // the four-product moment constants of every lane (aomarl_qf4_host.h), checked against M and S in double
    float qtab[64 * 8];
    if (!aomarl_qf4::build_table(qtab)) return create_refuse(P, "create: quadratic-form constants");
    CP_OWN(float, qtab, 64 * 8, qf_tab);
  }
  CP_OWN(uint16_t, tmask.data(), tmask.size(), tile_mask);
  CP_TRY(create_plan_tt_planes(d, P));
  s.fused_ok = 1; s.ntiles = nt;
  create_plan_otf(P, nt);
  return true;
}

// The plan of a descriptor, or its refusal (false: P.msg).
static inline bool create_plan(const aomarl_desc *d, CreatePlan &P) {
  if (!d) return create_refuse(P, "aomarl_create: null argument");
  if (d->abi_version != AOMARL_ABI_VERSION)
    return create_refuse(P, "aomarl_create: ABI version %d, library is %d", d->abi_version, AOMARL_ABI_VERSION);
  if (d->nlayers < 0 || d->nlayers > AOMARL_MAX_LAYERS) return create_refuse(P, "nlayers out of range");
  if (d->ndm < 1 || d->ndm > AOMARL_MAX_DMS) return create_refuse(P, "ndm out of range");
  if (d->n <= 0 || d->pupdiam <= 0 || d->n < d->pupdiam) return create_refuse(P, "bad pupil sizes");
  if (d->pupdiam % 4 || d->n % 4) return create_refuse(P, "pupil grid sizes must be multiples of 4");
  if (d->npsf <= 0 || (d->npsf & (d->npsf - 1))) return create_refuse(P, "npsf must be a power of two");
  if (!(d->strehl_halfwin == 4 || d->strehl_halfwin == 8 || d->strehl_halfwin == 16))
    return create_refuse(P, "strehl_halfwin must be 4, 8 or 16");
  DevSys &s = P.sys;
  memset(&s, 0, sizeof(s));
  s.n = d->n; s.pupdiam = d->pupdiam;
  CP_REF(float, d->mpupil, (size_t)d->n * d->n, mpupil);
  CP_REF(float, d->spupil, (size_t)d->pupdiam * d->pupdiam, spupil);
  P.host.h_spupil.assign(d->spupil, d->spupil + (size_t)d->pupdiam * d->pupdiam);
  std::vector<int32_t> sub;
  CP_TRY(create_plan_wfs(d, P, sub));
  CP_TRY(create_plan_layers(d, P));
  // DMs
  s.ndm = d->ndm;
  long long soff = 0; int coff = 0;
  for (int k = 0; k < d->ndm; k++) CP_TRY(create_plan_dm(d, k, P, soff, coff));
  s.shape_stride = soff;
  if (coff != d->nactu) return create_refuse(P, "sum of DM actuators (%d) != nactu (%d)", coff, d->nactu);
  if (d->nslope != 2 * d->nvalid) return create_refuse(P, "nslope must be 2*nvalid");
  s.nactu = d->nactu; s.nslope = d->nslope;
  P.production_layout = d->ndm == 2 && d->dms[0].type == AOMARL_DM_PZT && d->dms[1].type == AOMARL_DM_TT &&
                        (d->nlayers == 1 || d->nlayers == 3);
  CP_TRY(create_plan_target(d, P));
  P.host.gain = d->gain; P.host.delay = d->delay;
  if (P.host.delay < 0.f || P.host.delay > 2.f) return create_refuse(P, "delay must be in [0, 2]");
  return create_plan_frame(d, P, sub);
}

#undef CP_TRY
#undef CP_REF
#undef CP_OWN
