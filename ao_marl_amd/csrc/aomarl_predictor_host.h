// aomarl_predictor_host.h -- the host half of the modal predictor (aomarl_predictor.hip): the validation of the desc and
// of the state a caller hands to aomarl_predictor_set, and the two per-frame decisions the host takes from its counters
// alone.  Plain C++ without a HIP call and without a global, so that it also compiles into a stand-alone host program
// (predictor_host_check.cpp) that runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "../../include/aomarl.h"
#include "aomarl_predictor_fn.h"

static inline std::string pr_fmt(const char *fmt, double a = 0, double b = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b);
  return std::string(buf);
}

// 0 when the desc can be used; otherwise 1 and `err` names the field
static inline int pr_validate(const aomarl_predictor_desc *d, std::string &err) {
  if (!d) { err = "predictor_create: null desc"; return 1; }
  if (d->nenv < 1 || d->nmodes < 1)
    { err = pr_fmt("predictor_create: nenv = %.0f, nmodes = %.0f: both must be positive", d->nenv, d->nmodes); return 1; }
  if ((long long)d->nenv * d->nmodes > 0x7fffffffLL)
    { err = pr_fmt("predictor_create: nenv * nmodes = %.0f series exceed 2^31 - 1", (double)d->nenv * d->nmodes); return 1; }
  if (d->order < 1 || d->order > PR_MAXORDER)
    { err = pr_fmt("predictor_create: order = %.0f: 1..%.0f past values", d->order, PR_MAXORDER); return 1; }
  if (d->nskip < 0) { err = pr_fmt("predictor_create: nskip = %.0f must not be negative", d->nskip); return 1; }
  if (!(d->delay >= 0.f && d->delay <= 2.f))
    { err = pr_fmt("predictor_create: delay = %g: the delay line holds two frames (0 <= delay <= 2)", d->delay); return 1; }
  if (!(d->forget > 0.0 && d->forget <= 1.0)) { err = pr_fmt("predictor_create: forget = %g: in (0, 1]", d->forget); return 1; }
  if (!(d->p0 > 0.0) || !isfinite(d->p0)) { err = pr_fmt("predictor_create: p0 = %g: positive and finite", d->p0); return 1; }
  return 0;
}

// theta [nseries][order], P [nseries][order][order] (full) as a caller hands them to aomarl_predictor_set: all finite,
// P symmetric (bit for bit: only its upper triangle is kept) with a positive diagonal.  Either may be null.
static inline int pr_validate_set(long long nseries, int order, const double *theta, const double *P, std::string &err) {
  if (theta)
    for (long long i = 0; i < nseries * order; i++)
      if (!isfinite(theta[i])) { err = pr_fmt("predictor_set: theta[%.0f] is not finite", (double)i); return 1; }
  if (P)
    for (long long s = 0; s < nseries; s++) {
      const double *Ps = P + s * order * order;
      for (int i = 0; i < order; i++) {
        for (int j = 0; j < order; j++) {
          if (!isfinite(Ps[i * order + j]))
            { err = pr_fmt("predictor_set: P of series %.0f has a non-finite entry in row %.0f", (double)s, i); return 1; }
          if (Ps[i * order + j] != Ps[j * order + i])
            { err = pr_fmt("predictor_set: P of series %.0f is not symmetric (row %.0f)", (double)s, i); return 1; }
        }
        if (!(Ps[i * order + i] > 0.0))
          { err = pr_fmt("predictor_set: P of series %.0f has a diagonal entry that is not positive (row %.0f)", (double)s, i); return 1; }
      }
    }
  return 0;
}

// the counters of one predictor; all the host keeps per frame
struct PrCounts {
  long long total = 0, since = 0, learned = 0;      // frames pushed; since the last restart; frames that updated theta
};
// `n` frames are about to be pushed: the first one's index since the restart; the counters move on
static inline long long pr_advance(PrCounts &k, int n, int order, bool learning) {
  const long long f0 = k.since;
  if (learning) {
    const long long first = f0 > order + 2 ? f0 : order + 2;      // the first frame of these that learns
    if (f0 + n > first) k.learned += f0 + n - first;
  }
  k.total += n; k.since += n;
  return f0;
}
