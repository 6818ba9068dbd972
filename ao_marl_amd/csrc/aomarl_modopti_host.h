// aomarl_modopti_host.h -- the host half of the modal-gain filter bank (aomarl_modopti.hip): the delay-line weights, the
// validation of the desc and the stability test of one mode's closed loop.  Plain C++ without a HIP call, so that it also
// compiles into a stand-alone host program (modopti_host_check.cpp) that runs it under the address and
// undefined-behaviour sanitizers.
//
// One mode of the loop (frame t = next_part_two then next_part_one; k_delay forms the voltage of frame t from the
// commands as do_control left them at frames t-1, t-2, t-3):
//     e[t] = x[t] - (wa c[t-1] + wb c[t-2] + wc c[t-3]),     c[t] = c[t-1] + g e[t]
//     E/X  = (1 - z^-1) / (1 + (g wa - 1) z^-1 + g wb z^-2 + g wc z^-3)
// The loop is stable when every root of  z^3 + (g wa - 1) z^2 + g wb z + g wc  lies inside the unit circle.
// g = 0 is the open loop: the pole at 1 is cancelled by the numerator (e = x, nothing grows), a legal candidate.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include "../../include/aomarl.h"

#define MO_MAXGAIN 4096

// the weights of aomarl_apply_control's delay line: voltage = wa com + wb com1 + wc com2
static inline void mo_delay_weights(double delay, double *wa, double *wb, double *wc) {
  if (delay <= 1.0) { *wa = 1.0 - delay; *wb = delay; *wc = 0.0; } else { *wa = 0.0; *wb = 2.0 - delay; *wc = delay - 1.0; }
}

// Jury's criterion for  z^3 + a1 z^2 + a2 z + a3  (leading coefficient 1): all roots strictly inside the unit circle.
// A vanishing a3 (and a2) only adds roots at 0: the same four inequalities then state the criterion of the quadratic
// (linear) factor.
static inline bool mo_jury3(double a1, double a2, double a3) {
  if (!(isfinite(a1) && isfinite(a2) && isfinite(a3))) return false;
  const double p1 = 1.0 + a1 + a2 + a3, pm1 = -1.0 + a1 - a2 + a3;
  return p1 > 0.0 && pm1 < 0.0 && fabs(a3) < 1.0 && fabs(a3 * a3 - 1.0) > fabs(a3 * a1 - a2);
}

// may gain g be returned as an optimum for this delay?
static inline bool mo_stable(double g, double delay) {
  if (!isfinite(g)) return false;
  if (g == 0.0) return true;
  double wa, wb, wc;
  mo_delay_weights(delay, &wa, &wb, &wc);
  return mo_jury3(g * wa - 1.0, g * wb, g * wc);
}

static inline std::string mo_fmt(const char *fmt, double a = 0, double b = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b);
  return std::string(buf);
}

// 0 when the desc can be used; otherwise 1 and `err` names the field
static inline int mo_validate(const aomarl_modopti_desc *d, std::string &err) {
  if (!d) { err = "modopti_create: null desc"; return 1; }
  if (d->nenv < 1 || d->nmodes < 1)
    { err = mo_fmt("modopti_create: nenv = %.0f, nmodes = %.0f: both must be positive", d->nenv, d->nmodes); return 1; }
  if ((long long)d->nenv * d->nmodes > 0x7fffffffLL)
    { err = mo_fmt("modopti_create: nenv * nmodes = %.0f series exceed 2^31 - 1", (double)d->nenv * d->nmodes); return 1; }
  if (d->ngain < 1 || d->ngain > MO_MAXGAIN)
    { err = mo_fmt("modopti_create: ngain = %.0f: 1..%.0f candidate gains", d->ngain, MO_MAXGAIN); return 1; }
  if (!d->gains) { err = "modopti_create: null gains"; return 1; }
  if (!(d->delay >= 0.f && d->delay <= 2.f))
    { err = mo_fmt("modopti_create: delay = %g: the delay line holds two frames (0 <= delay <= 2)", d->delay); return 1; }
  if (d->nskip < 0) { err = mo_fmt("modopti_create: nskip = %.0f must not be negative", (double)d->nskip); return 1; }
  for (int j = 0; j < d->ngain; j++)
    if (!isfinite(d->gains[j]))
      { err = mo_fmt("modopti_create: gains[%.0f] is not finite", j); return 1; }
  return 0;
}

// ------------------------------------------------------------------------------------------------- on-line form
// aomarl_modopti_online_*: the same bank fed one pseudo-open-loop frame at a time while the loop is closed.  The rules
// below are all the host decides per frame -- no device value is read back for them.
//   every frame:  the row enters a ring of `chunk` rows; J = forget J + e^2 for frames whose index since the last
//                 restart is >= nskip
//   apply:        every `period` frames (counted over all frames pushed), once at least one frame has entered J
//   the bank kernel consumes the ring when it is full or an apply is due (and before a restart or a read-out)
struct MoSchedule {
  int chunk = 1;
  long long period = 1, nskip = 0;
  long long total = 0, since = 0, counted = 0, updates = 0;      // frames pushed; since restart; entered J; applies
  int fill = 0;                                                  // rows waiting in the ring
};
struct MoAction {
  int slot = 0;            // the ring row this frame is written to
  int flush = 0;           // rows the bank kernel consumes behind this frame (0: none)
  long long t0 = 0;        // ... index since restart of the first of them
  bool apply = false;
};
// the frame about to be pushed: where it goes and what follows it
static inline MoAction mo_online_step(MoSchedule &s) {
  MoAction a;
  a.slot = s.fill;
  if (s.since >= s.nskip) s.counted++;
  s.fill++; s.total++; s.since++;
  a.apply = s.total % s.period == 0 && s.counted > 0;
  if (s.fill == s.chunk || a.apply) { a.flush = s.fill; a.t0 = s.since - s.fill; s.fill = 0; }
  if (a.apply) s.updates++;
  return a;
}
// rows still waiting (before a restart or a read-out): consumed, the ring empty afterwards
static inline MoAction mo_online_drain(MoSchedule &s) {
  MoAction a;
  a.flush = s.fill; a.t0 = s.since - s.fill; s.fill = 0;
  return a;
}
// an episode reset: the filter history and the transient counter start over (the caller drains first); J, G and the
// apply schedule go on
static inline void mo_online_restart(MoSchedule &s) { s.since = 0; }

#define MO_MAXCHUNK 32

static inline int mo_online_validate(const aomarl_modopti_online_desc *d, std::string &err) {
  if (!d) { err = "modopti_online_create: null desc"; return 1; }
  aomarl_modopti_desc b;
  b.nenv = d->nenv; b.nmodes = d->nmodes; b.ngain = d->ngain; b.nskip = d->nskip; b.delay = d->delay; b.gains = d->gains;
  if (mo_validate(&b, err)) { err.replace(0, strlen("modopti_create"), "modopti_online_create"); return 1; }
  if (d->chunk < 1 || d->chunk > MO_MAXCHUNK)
    { err = mo_fmt("modopti_online_create: chunk = %.0f: 1..%.0f rows in the ring", d->chunk, MO_MAXCHUNK); return 1; }
  if (d->period < 1) { err = mo_fmt("modopti_online_create: period = %.0f: at least one frame between applies", d->period); return 1; }
  if (d->pool != 0 && d->pool != 1) { err = mo_fmt("modopti_online_create: pool = %.0f: 1 (all environments) or 0", d->pool); return 1; }
  if (!(d->forget > 0.0 && d->forget <= 1.0)) { err = mo_fmt("modopti_online_create: forget = %g: in (0, 1]", d->forget); return 1; }
  if (!(d->beta > 0.0 && d->beta <= 1.0)) { err = mo_fmt("modopti_online_create: beta = %g: in (0, 1]", d->beta); return 1; }
  bool any = false;
  for (int j = 0; j < d->ngain; j++) any = any || mo_stable((double)d->gains[j], (double)d->delay);
  if (!any) { err = mo_fmt("modopti_online_create: no candidate gain is stable at delay = %g", d->delay); return 1; }
  if (d->G0) {
    const long long n = (long long)(d->pool ? 1 : d->nenv) * d->nmodes;
    for (long long i = 0; i < n; i++)
      if (!isfinite(d->G0[i])) { err = mo_fmt("modopti_online_create: G0[%.0f] is not finite", (double)i); return 1; }
  }
  return 0;
}
