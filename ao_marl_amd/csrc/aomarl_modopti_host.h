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
