// aomarl_mcao_host.h -- the host half of multi-conjugate AO (aomarl_mcao.hip): the validation of the desc, of the view
// and of the arguments of aomarl_mcao_apply / _reset / _add (every refusal by name), the plan of the launches and the add
// kernel's offset table.  Plain C++ without a HIP call and without a global, so that it also compiles into a stand-alone
// host program under the address and undefined-behaviour sanitizers (mcao_host_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/aomarl.h"

#define MCAO_TILE 32                 // k_mcao_shape: a workgroup owns a 32 x 32 tile of a mirror's plane
#define MCAO_CELLS 12                // ... and stages the 12 x 12 lattice cells that can reach it
#define MCAO_MAX_SS 128              // ... and the profile
#define MCAO_THREADS 256

static inline std::string mcao_fmt(const char *fmt, double a = 0, double b = 0, double c = 0, double d = 0) {
  char buf[320];
  snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  return std::string(buf);
}

// lattice cells along one axis that can reach a tile: the first one is first_cell(p0) (k_mcao_shape), the last one has
// its patch start at or below p0 + MCAO_TILE - 1
static inline int mcao_cells_needed(int ss, int pitch) { return (MCAO_TILE + ss - 2) / pitch + 2; }

// ---- create
static inline int mcao_validate_desc(const aomarl_mcao_desc *d, int nenv, const void *out, std::string &err) {
  if (!d) { err = "mcao_create: null desc"; return 1; }
  if (!out) { err = "mcao_create: null output pointer"; return 1; }
  if (d->nmirrors < 1 || d->nmirrors > AOMARL_MCAO_MAX_MIRRORS)
    { err = mcao_fmt("mcao_create: %.0f mirrors: 1..%.0f", d->nmirrors, AOMARL_MCAO_MAX_MIRRORS); return 1; }
  if (nenv < 1) { err = mcao_fmt("mcao_create: %.0f environments: at least one", nenv); return 1; }
  long long dmax = 0, ntot = 0;
  for (int m = 0; m < d->nmirrors; m++) {
    const aomarl_mcao_mirror &M = d->mirrors[m];
    if (!(M.alt >= 0.f) || !isfinite(M.alt))
      { err = mcao_fmt("mcao_create: mirror %.0f: alt = %g m: finite and not negative", m, M.alt); return 1; }
    if (!M.grid || !M.prof) { err = mcao_fmt("mcao_create: mirror %.0f: null grid / prof", m); return 1; }
    if (M.dim < 2 || M.dim > 32768 || M.pitch < 1 || M.ss < 1 || M.gw < 1 || M.gh < 1 || M.nact < 1 ||
        (long long)M.gw * M.gh > 0x7fffffffLL || M.nact > (long long)M.gw * M.gh)
      { err = mcao_fmt("mcao_create: mirror %.0f: dim = %.0f, pitch = %.0f, ss = %.0f: sizes must be positive (dim 2..32768, nact <= gw gh)", m, M.dim, M.pitch, M.ss); return 1; }
    if (M.ss > MCAO_MAX_SS || mcao_cells_needed(M.ss, M.pitch) > MCAO_CELLS)
      { err = mcao_fmt("mcao_create: mirror %.0f: a profile of ss = %.0f pixels at pitch %.0f is larger than the shape kernel's LDS patch (%.0f lattice cells per axis, ss <= 128)", m, M.ss, M.pitch, MCAO_CELLS); return 1; }
    if (M.i1min < 0 || M.j1min < 0 || (long long)M.i1min + (long long)M.pitch * (M.gw - 1) + M.ss > M.dim ||
        (long long)M.j1min + (long long)M.pitch * (M.gh - 1) + M.ss > M.dim)
      { err = mcao_fmt("mcao_create: mirror %.0f: the lattice leaves the plane (origin (%.0f, %.0f), %.0f pixels)", m, M.i1min, M.j1min, M.dim); return 1; }
    for (long long q = 0; q < (long long)M.gw * M.gh; q++)
      if (M.grid[q] < -1 || M.grid[q] >= M.nact)
        { err = mcao_fmt("mcao_create: mirror %.0f: grid entry %.0f = %.0f outside -1..%.0f", m, (double)q, M.grid[q], M.nact - 1); return 1; }
    for (int t = 0; t < M.ss; t++)
      if (!isfinite(M.prof[t])) { err = mcao_fmt("mcao_create: mirror %.0f: prof[%.0f] is not finite", m, t); return 1; }
    dmax = M.dim > dmax ? M.dim : dmax;
    ntot += M.nact;
  }
  if ((long long)nenv * d->nmirrors * dmax * dmax > 0x7fffffffLL || (long long)nenv * ntot > 0x7fffffffLL)
    { err = mcao_fmt("mcao_create: the planes of %.0f environments and %.0f mirrors of %.0f pixels exceed 2^31 - 1 elements", nenv, d->nmirrors, (double)dmax); return 1; }
  return 0;
}

// ---- apply / reset / add: the environments of the range.  who: the entry point's name in the message
static inline int mcao_validate_range(const char *who, int nenv, int env_begin, int env_count, std::string &err) {
  if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > nenv)
    { err = std::string(who) + mcao_fmt(": environments %.0f .. +%.0f of %.0f", env_begin, env_count, nenv); return 1; }
  return 0;
}

// ---- the view.  dims[m]: the side of mirror m's plane; nn: the side of the grid that looks.  The footprint of direction
// k on mirror m is the coordinate at the grid's corners, evaluated as the kernel evaluates it (float, one fused
// multiply-add).  max_dir: AOMARL_MCAO_MAX_DIRS for an add, the field's own limit for an attached field.
static inline int mcao_validate_view(const char *who, const aomarl_mcao_view *v, int nmirrors, const int *dims, int nn,
                                     int max_dir, std::string &err) {
  const std::string w(who);
  if (!v) { err = w + ": null view"; return 1; }
  if (v->ndir < 1 || v->ndir > max_dir) { err = w + mcao_fmt(": %.0f directions: 1..%.0f", v->ndir, max_dir); return 1; }
  if (!v->off || !v->dm1) { err = w + ": null off / dm1"; return 1; }
  const float c = 0.5f * (float)(nn - 1);
  for (int k = 0; k < v->ndir; k++)
    for (int m = 0; m < nmirrors; m++) {
      const float g = v->dm1[k * nmirrors + m];
      const float *o = v->off + 2 * (k * nmirrors + m);
      if (!isfinite(o[0]) || !isfinite(o[1]))
        { err = w + mcao_fmt(": off of direction %.0f, mirror %.0f is not finite", k, m); return 1; }
      if (!(g > -1.f) || !(g <= 0.f))
        { err = w + mcao_fmt(": dm1 of direction %.0f, mirror %.0f = %g: -alt / gsalt must lie in (-1, 0]", k, m, g); return 1; }
      for (int ax = 0; ax < 2; ax++)
        for (int corner = 0; corner < 2; corner++) {
          const float x = corner ? (float)(nn - 1) : 0.f;
          const float f = fmaf(g, x - c, x + o[ax]);
          if (!(f >= 0.f) || !(f <= (float)(dims[m] - 1)))
            { err = w + mcao_fmt(": the footprint of direction %.0f leaves mirror %.0f: coordinate %.2f outside [0, %.0f] (build the mirror for a larger field radius)", k, m, f, dims[m] - 1); return 1; }
        }
    }
  return 0;
}

// ---- a science field that sees the mirrors (aomarl_field_attach_mirrors): one entry of the view per direction of the
// field, natural stars (dm1 = 0), each footprint on the pupil grid inside every plane
static inline int mcao_validate_attach(const aomarl_mcao_view *v, int field_ndir, int nmirrors, const int *dims, int pupdiam,
                                       std::string &err) {
  const char *who = "field_attach_mirrors";
  if (mcao_validate_view(who, v, nmirrors, dims, pupdiam, 0x7fffffff, err)) return 1;
  if (v->ndir != field_ndir)
    { err = std::string(who) + mcao_fmt(": the view has %.0f directions, the field %.0f", v->ndir, field_ndir); return 1; }
  for (int i = 0; i < v->ndir * nmirrors; i++)
    if (v->dm1[i] != 0.f)
      { err = std::string(who) + mcao_fmt(": dm1 of direction %.0f, mirror %.0f = %g: a science direction is a natural star (dm1 = 0)", i / nmirrors, i % nmirrors, v->dm1[i]); return 1; }
  return 0;
}

static inline int mcao_validate_add(const aomarl_mcao_view *v, const void *planes, int ndir, int nn, int n, int pupdiam,
                                    int nmirrors, const int *dims, int nenv, int env_begin, int env_count, int flags,
                                    int known_flags, std::string &err) {
  if (!planes) { err = "mcao_add: null planes"; return 1; }
  if (ndir < 1 || ndir > AOMARL_MCAO_MAX_DIRS) { err = mcao_fmt("mcao_add: %.0f directions: 1..%.0f", ndir, AOMARL_MCAO_MAX_DIRS); return 1; }
  if (nn != n && nn != pupdiam)
    { err = mcao_fmt("mcao_add: a grid of %.0f pixels: the sensor's (%.0f) or the pupil's (%.0f)", nn, n, pupdiam); return 1; }
  if (mcao_validate_view("mcao_add", v, nmirrors, dims, nn, AOMARL_MCAO_MAX_DIRS, err)) return 1;
  if (v->ndir != ndir) { err = mcao_fmt("mcao_add: the view has %.0f directions, the planes %.0f", v->ndir, ndir); return 1; }
  if (mcao_validate_range("mcao_add", nenv, env_begin, env_count, err)) return 1;
  if (flags & ~known_flags) { err = mcao_fmt("mcao_add: unknown flags %.0f", flags); return 1; }
  if ((long long)nenv * ndir * nn * nn > 0x7fffffffLL)
    { err = mcao_fmt("mcao_add: the planes of %.0f environments and %.0f directions exceed 2^31 - 1 elements", nenv, ndir); return 1; }
  return 0;
}

// direction slots of the add kernel's instantiation for K directions: the next power of two
static inline int mcao_slots(int K) {
  int kt = 1;
  while (kt < K) kt *= 2;
  return kt;
}

// ---- the plan of aomarl_mcao_apply's shape launch: mirror m's tiles are blocks [first[m], first[m] + tx[m] ty[m])
struct McaoPlan { int nmirrors, tx[AOMARL_MCAO_MAX_MIRRORS], first[AOMARL_MCAO_MAX_MIRRORS + 1]; };
static inline McaoPlan mcao_plan(const int *dims, int nmirrors) {
  McaoPlan p;
  memset(&p, 0, sizeof(p));
  p.nmirrors = nmirrors;
  for (int m = 0; m < nmirrors; m++) {
    p.tx[m] = (dims[m] + MCAO_TILE - 1) / MCAO_TILE;
    p.first[m + 1] = p.first[m] + p.tx[m] * p.tx[m];
  }
  return p;
}

// ---- the add kernel's argument: offsets [mirror][direction], the mirrors outer as the kernel walks them; the slots past
// the view's directions keep zero offsets
struct McaoAddArgs {
  float ox[AOMARL_MCAO_MAX_MIRRORS][AOMARL_MCAO_MAX_DIRS], oy[AOMARL_MCAO_MAX_MIRRORS][AOMARL_MCAO_MAX_DIRS];
  float dm1[AOMARL_MCAO_MAX_MIRRORS][AOMARL_MCAO_MAX_DIRS];
};
static inline McaoAddArgs mcao_add_args(const aomarl_mcao_view *v, int nmirrors) {
  McaoAddArgs a;
  memset(&a, 0, sizeof(a));
  for (int m = 0; m < nmirrors; m++)
    for (int k = 0; k < v->ndir; k++) {
      a.ox[m][k] = v->off[2 * (k * nmirrors + m)];
      a.oy[m][k] = v->off[2 * (k * nmirrors + m) + 1];
      a.dm1[m][k] = v->dm1[k * nmirrors + m];
    }
  return a;
}
