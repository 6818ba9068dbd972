// aomarl_field_host.h -- the host half of the science field (aomarl_field.hip): the validation of the desc and of the
// arguments of aomarl_field_observe / _trace / _reset (every refusal by name), the plan of the launches (a field with more
// than AOMARL_FIELD_MAX_DIRS directions runs as consecutive launches) and the kernel's offset table.  Plain C++ without a
// HIP call and without a global, so that it also compiles into a stand-alone host program under the address and
// undefined-behaviour sanitizers (field_host_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/aomarl.h"

#define FIELD_THREADS 256
#define FIELD_MAX_LAYERS 8           // (AOMARL_MAX_LAYERS)
#define FIELD_MAX_DMS 4              // (AOMARL_MAX_DMS)
#define FIELD_TW_LDS 2048             // k_field_rows keeps the twiddles in LDS up to this Npsf

static inline std::string field_fmt(const char *fmt, double a = 0, double b = 0, double c = 0, double d = 0) {
  char buf[320];
  snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  return std::string(buf);
}

// what the validation reads of the context: the screens' sides, the pupil grid, the PSF window, the mirrors' supports and
// their offsets on the target's path
struct FieldSys {
  int nlayers, dims[FIELD_MAX_LAYERS];
  int pupdiam, hw;
  int ndm, dm_dim[FIELD_MAX_DMS];
  float dm_txo[FIELD_MAX_DMS], dm_tyo[FIELD_MAX_DMS];
};

// ---- create.  The footprint of direction d on layer l is the trace's coordinate at the pupil grid's corners, evaluated
// as the kernel evaluates it (float).  A mirror in the pupil (alt = 0) sits at (dim - pupdiam) / 2 on the target's path
// whatever the target's direction (geometry.target_layer_offsets); any other offset is a mirror at altitude seen off axis.
static inline int field_validate_desc(const aomarl_field_desc *d, const FieldSys &sy, int nenv, const void *out, std::string &err) {
  if (!d) { err = "field_create: null desc"; return 1; }
  if (!out) { err = "field_create: null output pointer"; return 1; }
  if (d->ndir < 1) { err = field_fmt("field_create: ndir = %.0f: at least one direction", d->ndir); return 1; }
  if (d->nlayers != sy.nlayers || d->nlayers < 0 || d->nlayers > FIELD_MAX_LAYERS)
    { err = field_fmt("field_create: offsets for %.0f layers, the context has %.0f", d->nlayers, sy.nlayers); return 1; }
  if (!d->off) { err = "field_create: null off"; return 1; }
  if (nenv < 1) { err = field_fmt("field_create: %.0f environments: at least one", nenv); return 1; }
  if (!(d->inv_lambda > 0.f) || !isfinite(d->inv_lambda))
    { err = field_fmt("field_create: inv_lambda = %g per micron: positive and finite", d->inv_lambda); return 1; }
  if (sy.hw < 1 || 2 * sy.hw > FIELD_THREADS)
    { err = field_fmt("field_create: strehl_halfwin = %.0f: the window's side 2 hw must lie in 2..%.0f", sy.hw, FIELD_THREADS); return 1; }
  if ((long long)nenv * d->ndir * sy.pupdiam * sy.pupdiam > 0x7fffffffLL)
    { err = field_fmt("field_create: the planes of %.0f environments and %.0f directions exceed 2^31 - 1 elements", nenv, d->ndir); return 1; }
  for (int k = 0; k < sy.ndm; k++) {
    const float want = 0.5f * (float)(sy.dm_dim[k] - sy.pupdiam);
    if (sy.dm_txo[k] != want || sy.dm_tyo[k] != want)
      { err = field_fmt("field_create: mirror %.0f is not in the pupil (its offset on the target's path is (%g, %g), a mirror at altitude 0 has %g): mirrors at altitude are not covered", k, sy.dm_txo[k], sy.dm_tyo[k], want); return 1; }
  }
  for (int k = 0; k < d->ndir; k++)
    for (int l = 0; l < d->nlayers; l++) {
      const float *o = d->off + 2 * ((size_t)k * d->nlayers + l);
      if (!isfinite(o[0]) || !isfinite(o[1]))
        { err = field_fmt("field_create: off of direction %.0f, layer %.0f is not finite", k, l); return 1; }
      for (int ax = 0; ax < 2; ax++)
        for (int corner = 0; corner < 2; corner++) {
          const float f = (corner ? (float)(sy.pupdiam - 1) : 0.f) + o[ax];
          if (!(f >= 0.f) || !(f <= (float)(sy.dims[l] - 1)))
            { err = field_fmt("field_create: the footprint of direction %.0f leaves screen %.0f: coordinate %.2f outside [0, %.0f] (declare the field in the parameter file)", k, l, f, sy.dims[l] - 1); return 1; }
        }
    }
  return 0;
}

// ---- observe / trace / reset.  who: the entry point's name in the message
static inline int field_validate_call(const char *who, int field_nenv, int state_nenv, int env_begin, int env_count, int flags,
                                      int known_flags, std::string &err) {
  if (state_nenv != field_nenv)
    { err = std::string(who) + field_fmt(": the field has %.0f environments, the state %.0f", field_nenv, state_nenv); return 1; }
  if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > field_nenv)
    { err = std::string(who) + field_fmt(": environments %.0f .. +%.0f of %.0f", env_begin, env_count, field_nenv); return 1; }
  if (flags & ~known_flags) { err = std::string(who) + field_fmt(": unknown flags %.0f", flags); return 1; }
  return 0;
}

// ---- the plan: launch i covers directions [first, first + count), count <= AOMARL_FIELD_MAX_DIRS
struct FieldLaunch { int first, count; };
static inline std::vector<FieldLaunch> field_plan(int ndir) {
  std::vector<FieldLaunch> p;
  for (int d0 = 0; d0 < ndir; d0 += AOMARL_FIELD_MAX_DIRS)
    p.push_back({d0, ndir - d0 < AOMARL_FIELD_MAX_DIRS ? ndir - d0 : AOMARL_FIELD_MAX_DIRS});
  return p;
}
// directions that share the workspaces of one launch
static inline int field_chunk(int ndir) { return ndir < AOMARL_FIELD_MAX_DIRS ? ndir : AOMARL_FIELD_MAX_DIRS; }

// direction slots of the kernel instantiation that runs a launch of `count` directions: the next power of two
static inline int field_slots(int count) {
  int kt = 1;
  while (kt < count) kt *= 2;
  return kt;
}

// the kernels' argument: offsets [layer][direction of the launch], the layers outer as the kernels walk them
struct FieldArgs { float ox[FIELD_MAX_LAYERS][AOMARL_FIELD_MAX_DIRS], oy[FIELD_MAX_LAYERS][AOMARL_FIELD_MAX_DIRS]; };
// frac_x / frac_y: what is added per layer (the wind accumulators' remainder with "subpixel_flow"), or null
static inline FieldArgs field_args(const float *off, int nlayers, const FieldLaunch &L, const float *frac_x, const float *frac_y) {
  FieldArgs a;
  memset(&a, 0, sizeof(a));
  for (int l = 0; l < nlayers; l++)
    for (int k = 0; k < L.count; k++) {
      const float *o = off + 2 * ((size_t)(L.first + k) * nlayers + l);
      a.ox[l][k] = frac_x ? o[0] + frac_x[l] : o[0];
      a.oy[l][k] = frac_y ? o[1] + frac_y[l] : o[1];
    }
  return a;
}

// ---- mirrors at altitude attached to the field (aomarl_field_attach_mirrors; the view's validation is
// mcao_validate_attach, aomarl_mcao_host.h).  The ALT instantiations of the kernels take a FieldMirArgs behind their other
// arguments, the others an empty struct: planes [nenv][nmirrors][stride] of the attached object, mirror m's plane of side
// dim[m], the offsets [mirror][direction of the launch] (dm1 = 0: natural stars).
#define FIELD_MAX_ALT 2              // (AOMARL_MCAO_MAX_MIRRORS)
struct FieldNoMirrors {};
struct FieldMirArgs {
  const float *planes;
  int nmirrors, stride, dim[FIELD_MAX_ALT];
  float ox[FIELD_MAX_ALT][AOMARL_FIELD_MAX_DIRS], oy[FIELD_MAX_ALT][AOMARL_FIELD_MAX_DIRS];
};
template <bool ALT> struct FieldMir { typedef FieldNoMirrors type; };
template <> struct FieldMir<true> { typedef FieldMirArgs type; };
// base: planes, nmirrors, stride, dim filled in; off: HOST [ndir][nmirrors][2]
static inline FieldMirArgs field_mir_args(const FieldMirArgs &base, const float *off, const FieldLaunch &L) {
  FieldMirArgs a = base;
  memset(a.ox, 0, sizeof(a.ox));
  memset(a.oy, 0, sizeof(a.oy));
  for (int m = 0; m < base.nmirrors; m++)
    for (int k = 0; k < L.count; k++) {
      a.ox[m][k] = off[2 * ((size_t)(L.first + k) * base.nmirrors + m)];
      a.oy[m][k] = off[2 * ((size_t)(L.first + k) * base.nmirrors + m) + 1];
    }
  return a;
}
