// modopti_host_check.cpp -- a stand-alone host program around aomarl_modopti_host.h (the delay weights, the desc
// validation and the stability test of aomarl_modopti_create), meant to be built with the address and
// undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o modopti_host_check modopti_host_check.cpp
// No GPU, no HIP.  It checks the stability test against the closed-form limits of delays 0, 1 and 2 and, on a grid of
// delays and gains, against the loop run for 4000 frames on an impulse; it feeds the validator every malformed desc it
// is written to refuse.  Exit status 0: all held.
//     modopti_host_check stable <delay> <g> [<g> ...]     prints 1 or 0 per gain (tests/test_modal_gains.py compares
//                                                          them with the roots numpy finds)
#include "aomarl_modopti_host.h"
#include <stdlib.h>
#include <vector>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

// the loop on x = (1, 0, 0, ...): the largest |e| of the last quarter against the largest of the first
static bool decays(double g, double delay) {
  double wa, wb, wc;
  mo_delay_weights(delay, &wa, &wb, &wc);
  const int T = 4000;
  double c0 = 0, c1 = 0, c2 = 0, head = 0, tail = 0;
  for (int t = 0; t < T; t++) {
    const double e = (t == 0 ? 1.0 : 0.0) - (wa * c0 + wb * c1 + wc * c2);
    const double cn = c0 + g * e;
    c2 = c1; c1 = c0; c0 = cn;
    if (!isfinite(e)) return false;
    if (t < T / 4) head = fmax(head, fabs(e));
    if (t >= 3 * T / 4) tail = fmax(tail, fabs(e));
  }
  return tail < 1e-3 * head;
}

int main(int argc, char **argv) {
  if (argc >= 4 && std::string(argv[1]) == "stable") {
    const double delay = atof(argv[2]);
    for (int i = 3; i < argc; i++) printf("%d\n", mo_stable(atof(argv[i]), delay) ? 1 : 0);
    return 0;
  }
  double wa, wb, wc;
  mo_delay_weights(0.0, &wa, &wb, &wc);  REQUIRE(wa == 1.0 && wb == 0.0 && wc == 0.0);
  mo_delay_weights(0.5, &wa, &wb, &wc);  REQUIRE(wa == 0.5 && wb == 0.5 && wc == 0.0);
  mo_delay_weights(1.0, &wa, &wb, &wc);  REQUIRE(wa == 0.0 && wb == 1.0 && wc == 0.0);
  mo_delay_weights(1.5, &wa, &wb, &wc);  REQUIRE(wa == 0.0 && wb == 0.5 && wc == 0.5);
  mo_delay_weights(2.0, &wa, &wb, &wc);  REQUIRE(wa == 0.0 && wb == 0.0 && wc == 1.0);
  // closed-form limits: delay 0: 0 < g < 2; delay 1: g < 1; delay 2: g < (sqrt 5 - 1) / 2
  const double lim[3] = {2.0, 1.0, 0.5 * (sqrt(5.0) - 1.0)};
  for (int d = 0; d < 3; d++) {
    REQUIRE(mo_stable(lim[d] * (1.0 - 1e-3), (double)d));
    REQUIRE(!mo_stable(lim[d] * (1.0 + 1e-3), (double)d));
    REQUIRE(mo_stable(0.0, (double)d));              // the open loop: the pole at 1 is cancelled, a legal candidate
    REQUIRE(mo_stable(1e-6, (double)d));
    REQUIRE(!mo_stable(-1e-6, (double)d));
    REQUIRE(!mo_stable(NAN, (double)d) && !mo_stable(INFINITY, (double)d));
  }
  // poles exactly ON the circle (the last entry of the default grid at delay 1, ...) are not stable
  REQUIRE(!mo_stable(1.0, 1.0) && !mo_stable(2.0, 0.0) && !mo_stable(2.0, 0.5));
  // against the loop itself, away from the boundary (where 4000 frames decide)
  int nst = 0, nun = 0;
  for (int di = 0; di <= 8; di++)
    for (int gi = 1; gi <= 220; gi++) {
      const double delay = 0.25 * di, g = 0.01 * gi;
      const bool s = mo_stable(g, delay), s_lo = mo_stable(g * 0.97, delay), s_hi = mo_stable(g * 1.03, delay);
      if (s != s_lo || s != s_hi) continue;          // within 3 % of the limit
      REQUIRE(decays(g, delay) == s);
      (s ? nst : nun)++;
    }
  REQUIRE(nst > 300 && nun > 300);
  // every refusal of the validator, by the field it names
  std::string err;
  const float gains[3] = {0.f, 0.5f, 1.f};
  aomarl_modopti_desc ok;
  ok.nenv = 3; ok.nmodes = 5; ok.ngain = 3; ok.nskip = 10; ok.delay = 1.f; ok.gains = gains;
  REQUIRE(mo_validate(&ok, err) == 0);
  REQUIRE(mo_validate(nullptr, err) == 1);
  { aomarl_modopti_desc d = ok; d.nenv = 0; REQUIRE(mo_validate(&d, err) == 1 && err.find("nenv") != std::string::npos); }
  { aomarl_modopti_desc d = ok; d.nmodes = -1; REQUIRE(mo_validate(&d, err) == 1 && err.find("nmodes") != std::string::npos); }
  { aomarl_modopti_desc d = ok; d.nenv = 65536; d.nmodes = 65536; REQUIRE(mo_validate(&d, err) == 1 && err.find("2^31") != std::string::npos); }
  { aomarl_modopti_desc d = ok; d.ngain = 0; REQUIRE(mo_validate(&d, err) == 1 && err.find("ngain") != std::string::npos); }
  { aomarl_modopti_desc d = ok; d.ngain = MO_MAXGAIN + 1; REQUIRE(mo_validate(&d, err) == 1 && err.find("ngain") != std::string::npos); }
  { aomarl_modopti_desc d = ok; d.gains = nullptr; REQUIRE(mo_validate(&d, err) == 1 && err.find("null gains") != std::string::npos); }
  { aomarl_modopti_desc d = ok; d.nskip = -1; REQUIRE(mo_validate(&d, err) == 1 && err.find("nskip") != std::string::npos); }
  const float delays[] = {-0.1f, 2.5f, NAN};
  for (float dl : delays) { aomarl_modopti_desc d = ok; d.delay = dl; REQUIRE(mo_validate(&d, err) == 1 && err.find("delay") != std::string::npos); }
  const float bad[] = {NAN, INFINITY, -INFINITY};
  for (float b : bad) {
    float gg[3] = {0.f, b, 1.f};
    aomarl_modopti_desc d = ok; d.gains = gg;
    REQUIRE(mo_validate(&d, err) == 1 && err.find("gains[1]") != std::string::npos);
  }
  { const float neg[3] = {-0.5f, 0.5f, 3.f}; aomarl_modopti_desc d = ok; d.gains = neg; REQUIRE(mo_validate(&d, err) == 0); }
  printf("modopti_host_check: ok\n");
  return 0;
}
