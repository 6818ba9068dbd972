// aomarl_dmreg_host.h -- the host half of the mirror mis-registration (aomarl_capi_dmreg.hip): the four-parameter form,
// the validation of the table rows, of the ranges and of the context's state, and the bound on the coordinates an
// accepted table can produce.  Plain C++ without a HIP call and without a global, so that it also compiles into a
// stand-alone host program (dmreg_host_check.cpp) that runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

// one row of the table: A00, A01, A10, A11, tx, ty
#define DMREG_ROW 6
#define DMREG_A_MAX 4.0        // |A_ij|
#define DMREG_DET_MIN 0.25     // |det A|
#define DMREG_DET_MAX 4.0
#define DMREG_T_DIMS 4.0       // |t| in sides of the mirror's plane
// what the kernel's float -> int conversion of a coordinate must stay inside (far inside int32)
#define DMREG_COORD_MAX 1073741824.0

static inline std::string dmreg_fmt(const char *fmt, double a = 0, double b = 0, double c = 0, double d = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  return std::string(buf);
}

static inline void dmreg_identity(float *At, long long rows) {
  for (long long i = 0; i < rows; i++) {
    float *r = At + i * DMREG_ROW;
    r[0] = 1.f; r[1] = 0.f; r[2] = 0.f; r[3] = 1.f; r[4] = 0.f; r[5] = 0.f;
  }
}

// The four-parameter form (dx, dy in pupil pixels): the surface seen in the pupil is the registered one magnified by G
// about the pupil centre, rotated by theta from x towards y, then shifted by (dx, dy); the SAMPLE position is the
// inverse map: A = (1 / G) [[cos, sin], [-sin, cos]], t = -A (dx, dy).  In double, rounded once to fp32.
static inline void dmreg_affine(double dx, double dy, double theta, double G, float *row) {
  const double c = cos(theta) / G, s = sin(theta) / G;
  const double a00 = c, a01 = s, a10 = -s, a11 = c;
  row[0] = (float)a00; row[1] = (float)a01; row[2] = (float)a10; row[3] = (float)a11;
  row[4] = (float)(-(a00 * dx + a01 * dy)); row[5] = (float)(-(a10 * dx + a11 * dy));
}

// the largest |coordinate| any accepted row can give on a grid of nn pixels for a mirror of `dim` pixels at offset `off`
static inline double dmreg_coord_bound(int nn, double off, int dim) {
  const double c = 0.5 * (nn - 1);
  return fabs(c + off) + 2.0 * DMREG_A_MAX * c + DMREG_T_DIMS * dim;
}

// 0 when a table can be created for these sizes; otherwise 1 and `err` names the reason
static inline int dmreg_validate_create(int nenv, int ndm, std::string &err) {
  if (nenv < 1 || nenv > 65535) { err = dmreg_fmt("dmreg_create: nenv = %.0f: 1..65535 environments", nenv); return 1; }
  if (ndm < 1) { err = dmreg_fmt("dmreg_create: the context has %.0f mirrors", ndm); return 1; }
  return 0;
}
static inline int dmreg_validate_geometry(int nn, double xoff, double yoff, int dim, int dm, std::string &err) {
  if (!isfinite(xoff) || !isfinite(yoff) || dim < 1 ||
      !(dmreg_coord_bound(nn, xoff, dim) < DMREG_COORD_MAX) || !(dmreg_coord_bound(nn, yoff, dim) < DMREG_COORD_MAX))
    { err = dmreg_fmt("dmreg_create: mirror %.0f (dim %.0f) on a grid of %.0f pixels: coordinates would leave the int32 range", dm, dim, nn); return 1; }
  return 0;
}

// a context with a pipelined frame or a prefetched reset in flight
static inline int dmreg_validate_ctx(bool pipelined_frame, bool prefetched_reset, const char *who, std::string &err) {
  if (pipelined_frame)
    { err = std::string(who) + ": a pipelined frame is in flight (aomarl_set_frame_pipeline): the frame kernel samples registered mirrors -- reset first"; return 1; }
  if (prefetched_reset)
    { err = std::string(who) + ": a prefetched reset is in flight (aomarl_reset_prefetch_begin): aomarl_reset_prefetch_cancel first"; return 1; }
  return 0;
}

static inline int dmreg_validate_range(int nenv, int ndm, int env_begin, int env_count, int dm, const char *who, std::string &err) {
  if (env_begin < 0 || env_count < 1 || (long long)env_begin + env_count > nenv)
    { err = std::string(who) + dmreg_fmt(": environments %.0f .. +%.0f of %.0f", env_begin, env_count, nenv); return 1; }
  if (dm < 0 || dm >= ndm) { err = std::string(who) + dmreg_fmt(": mirror %.0f of %.0f", dm, ndm); return 1; }
  return 0;
}

// At [rows][6] for a mirror whose plane has `dim` pixels a side
static inline int dmreg_validate_rows(const float *At, int rows, int dim, std::string &err) {
  if (!At) { err = "dmreg_set: null table"; return 1; }
  for (int i = 0; i < rows; i++) {
    const float *r = At + (long long)i * DMREG_ROW;
    for (int j = 0; j < DMREG_ROW; j++)
      if (!isfinite(r[j])) { err = dmreg_fmt("dmreg_set: row %.0f entry %.0f is not finite", i, j); return 1; }
    for (int j = 0; j < 4; j++)
      if (fabs((double)r[j]) > DMREG_A_MAX)
        { err = dmreg_fmt("dmreg_set: row %.0f: |A| entry %.0f = %g exceeds %g", i, j, r[j], DMREG_A_MAX); return 1; }
    const double det = (double)r[0] * r[3] - (double)r[1] * r[2];
    if (!(fabs(det) >= DMREG_DET_MIN && fabs(det) <= DMREG_DET_MAX))
      { err = dmreg_fmt("dmreg_set: row %.0f: |det A| = %g outside [%g, %g]", i, fabs(det), DMREG_DET_MIN, DMREG_DET_MAX); return 1; }
    if (fabs((double)r[4]) > DMREG_T_DIMS * dim || fabs((double)r[5]) > DMREG_T_DIMS * dim)
      { err = dmreg_fmt("dmreg_set: row %.0f: |t| = (%g, %g) beyond %g pixels (4 dim)", i, r[4], r[5], DMREG_T_DIMS * dim); return 1; }
  }
  return 0;
}

static inline int dmreg_validate_trace(int nenv, int env_begin, int env_count, int target, int flags, int known_flags,
                                       std::string &err) {
  if (env_begin < 0 || env_count < 0 || (long long)env_begin + env_count > nenv)
    { err = dmreg_fmt("dmreg_trace: environments %.0f .. +%.0f of %.0f", env_begin, env_count, nenv); return 1; }
  if (target != 0 && target != 1) { err = dmreg_fmt("dmreg_trace: target = %.0f: 0 (sensor) or 1 (target)", target); return 1; }
  if (flags & ~known_flags) { err = dmreg_fmt("dmreg_trace: unknown flags %.0f", flags); return 1; }
  return 0;
}

// the sample position of pixel (x, y) in the order the kernel evaluates it (fp32): used by the host check to show
// that the identity row gives (x + ox, y + oy) exactly and that accepted rows stay inside the coordinate bound
static inline void dmreg_sample(const float *row, int nn, float ox, float oy, int x, int y, float *u, float *v) {
  const float c = 0.5f * (float)(nn - 1);
  const float dx = (float)x - c, dy = (float)y - c;
  *u = (c + ox) + (row[0] * dx + (row[1] * dy + row[4]));
  *v = (c + oy) + (row[2] * dx + (row[3] * dy + row[5]));
}

// bytes one environment's trace moves, from shapes alone: the windows of the screens the grid looks at (nn x nn floats a
// layer), the window of every mirror's plane it looks at near the identity (min(dim, nn)^2 floats; tip-tilt: two
// commands -- its two static planes are shared by all environments and counted once in `shared`), one store of the grid
static inline long long dmreg_trace_bytes(int nn, int nlayers, int ndm, const int *dim, const int *is_tt, long long *shared) {
  long long b = 4LL * nn * nn * nlayers + 4LL * nn * nn, sh = 0;
  for (int k = 0; k < ndm; k++) {
    const long long w = dim[k] < nn ? dim[k] : nn;
    if (is_tt[k]) { b += 8; sh += 8LL * w * w; }
    else b += 4LL * w * w;
  }
  if (shared) *shared = sh;
  return b;
}
