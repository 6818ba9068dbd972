// predictor_host_check.cpp -- a stand-alone host program around the host half of the modal predictor
// (aomarl_predictor_host.h: the validation of the desc and of aomarl_predictor_set's input, the frame counters) and around
// the per-series update itself (aomarl_predictor_fn.h, the text k_pred_step compiles), meant to be built with the address
// and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o predictor_host_check predictor_host_check.cpp
// No GPU, no HIP.  The update is run for every order 1 .. 8, with and without forgetting, learning and frozen, over a few
// hundred frames with a restart in the middle, against a plain-loop restatement (run-time order, the full matrix P)
// written below: theta, P, J, J0 and c to 1e-12 of their size.  Exit status 0: all held.
//     predictor_host_check run <order> <delay> <forget> <p0> <nskip> x0 x1 ...
// prints theta, the full P, J, J0 and every c of that series (for the test against the NumPy statement).
#include "aomarl_predictor_host.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static PredParams params(int n, double delay, double forget, double p0) {
  PredParams p;
  if (delay <= 1.0) { p.wa = 1.0 - delay; p.wb = delay; p.wc = 0.0; } else { p.wa = 0.0; p.wb = 2.0 - delay; p.wc = delay - 1.0; }
  p.forget = forget; p.iforget = 1.0 / forget; p.cap = n * p0;
  return p;
}

// the restatement: the law as the header's comment gives it, nothing shared with the header's code
struct Plain {
  int n;
  double wa, wb, wc, forget, p0, J = 0, J0 = 0;
  std::vector<double> th, P, past;      // P full [n][n]; past[k] = x[t-1-k], k < n + 2
  Plain(int n_, const PredParams &p, double p0_) : n(n_), wa(p.wa), wb(p.wb), wc(p.wc), forget(p.forget), p0(p0_) {
    th.assign(n, 0.0); th[0] = 1.0;
    P.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) P[(size_t)i * n + i] = p0;
    past.assign(n + 2, 0.0);
  }
  void restart() { past.assign(n + 2, 0.0); }
  double step(double x, bool count, bool learn) {
    std::vector<double> phi(n), q(n);
    double pred = 0;
    for (int i = 0; i < n; i++) { phi[i] = wa * past[i] + wb * past[i + 1] + wc * past[i + 2]; pred += th[i] * phi[i]; }
    const double eps = x - pred;
    if (count) { J = forget * J + eps * eps; J0 = forget * J0 + x * x; }
    if (learn) {
      double den = forget;
      for (int i = 0; i < n; i++) { q[i] = 0; for (int j = 0; j < n; j++) q[i] += P[(size_t)i * n + j] * phi[j]; }
      for (int i = 0; i < n; i++) den += phi[i] * q[i];
      for (int i = 0; i < n; i++) th[i] += q[i] * (eps / den);
      double tr = 0;
      for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) P[(size_t)i * n + j] = (P[(size_t)i * n + j] - q[i] * q[j] / den) / forget;
      for (int i = 0; i < n; i++) tr += P[(size_t)i * n + i];
      if (tr > n * p0) for (double &v : P) v *= n * p0 / tr;
    }
    double c = th[0] * x;
    for (int i = 1; i < n; i++) c += th[i] * past[i - 1];
    for (int k = n + 1; k > 0; k--) past[k] = past[k - 1];
    past[0] = x;
    return c;
  }
};

static bool close_to(double a, double b, double scale) { return fabs(a - b) <= 1e-12 * (scale > 1e-300 ? scale : 1.0); }

// a coloured series with an all-zero stretch, deterministic (no library generator: the same on every host)
static std::vector<float> series(int T, unsigned seed, bool zero) {
  std::vector<float> x(T, 0.f);
  if (zero) return x;
  unsigned s = seed * 2654435761u + 12345u;
  double a1 = 0, a2 = 0;
  for (int t = 0; t < T; t++) {
    s = s * 1664525u + 1013904223u; const double u = ((s >> 8) & 0xffff) / 65536.0 - 0.5;
    s = s * 1664525u + 1013904223u; const double v = ((s >> 8) & 0xffff) / 65536.0 - 0.5;
    const double a = 1.9 * a1 - 0.91 * a2 + 0.05 * u;
    a2 = a1; a1 = a;
    x[t] = (float)(a + 0.02 * v);
  }
  return x;
}

template <int N, bool FORGET> static int run_order(double delay, double forget, double p0, bool zero) {
  const int T = 400, nskip = 30, freeze_from = 330;
  const PredParams p = params(N, delay, forget, p0);
  PredSeries<N> s;
  pred_init(s, p0);
  Plain ref(N, p, p0);
  const std::vector<float> x = series(T, (unsigned)(N * 7 + (FORGET ? 1 : 0)), zero);
  PrCounts k;
  long long learned = 0;
  double cmax = 0;
  for (int t = 0; t < T; t++) {
    if (t == 170) { ref.restart(); for (int i = 0; i < N + 2; i++) s.xp[i] = 0.0; k.since = 0; }
    const bool learning = t < freeze_from;
    const long long f = pr_advance(k, 1, N, learning);
    const bool count = f >= nskip, learn = learning && f >= N + 2;
    learned += learn ? 1 : 0;
    const double c = pred_step<N, FORGET>(s, (double)x[t], p, count, learn);
    const double cr = ref.step((double)x[t], count, learn);
    cmax = fabs(cr) > cmax ? fabs(cr) : cmax;
    REQUIRE(isfinite(c) && close_to(c, cr, cmax));
  }
  REQUIRE(k.total == T && k.since == T - 170 && k.learned == learned);
  double tmax = 0, pmax = 0, tr = 0;
  for (int i = 0; i < N; i++) tmax = fabs(ref.th[i]) > tmax ? fabs(ref.th[i]) : tmax;
  for (double v : ref.P) pmax = fabs(v) > pmax ? fabs(v) : pmax;
  for (int i = 0; i < N; i++) REQUIRE(close_to(s.th[i], ref.th[i], tmax));
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++)
      REQUIRE(close_to(s.P[i <= j ? PR_IJ(N, i, j) : PR_IJ(N, j, i)], ref.P[(size_t)i * N + j], pmax));
  for (int i = 0; i < N; i++) tr += s.P[PR_IJ(N, i, i)];
  REQUIRE(tr > 0 && tr <= N * p0 * (1 + 1e-12));
  REQUIRE(close_to(s.J, ref.J, ref.J) && close_to(s.J0, ref.J0, ref.J0));
  if (zero) {
    REQUIRE(s.th[0] == 1.0 && s.J == 0.0 && cmax == 0.0);
    for (int i = 1; i < N; i++) REQUIRE(s.th[i] == 0.0);
  }
  return 0;
}

template <int N> static int run_all() {
  for (double delay : {0.0, 0.4, 1.0, 1.6, 2.0})
    for (int zero = 0; zero < 2; zero++) {
      REQUIRE((run_order<N, false>(delay, 1.0, 1e4, zero != 0) == 0));
      REQUIRE((run_order<N, true>(delay, 0.98, 1e4, zero != 0) == 0));
      REQUIRE((run_order<N, true>(delay, 1.0, 50.0, zero != 0) == 0));      // the FORGET text at forget = 1: the same numbers
    }
  return 0;
}

template <int N> static int print_run(double delay, double forget, double p0, long long nskip, int T, char **xs) {
  const PredParams p = params(N, delay, forget, p0);
  PredSeries<N> s;
  pred_init(s, p0);
  std::vector<float> c(T);
  for (int t = 0; t < T; t++) {
    const double x = (double)(float)atof(xs[t]);
    c[t] = (float)(forget != 1.0 ? pred_step<N, true>(s, x, p, t >= nskip, t >= N + 2) : pred_step<N, false>(s, x, p, t >= nskip, t >= N + 2));
  }
  for (int i = 0; i < N; i++) printf("%.17g\n", s.th[i]);
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) printf("%.17g\n", s.P[i <= j ? PR_IJ(N, i, j) : PR_IJ(N, j, i)]);
  printf("%.17g\n%.17g\n", s.J, s.J0);
  for (int t = 0; t < T; t++) printf("%.9g\n", (double)c[t]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 7 && !strcmp(argv[1], "run")) {
    const int n = atoi(argv[2]), T = argc - 7;
    const double delay = atof(argv[3]), forget = atof(argv[4]), p0 = atof(argv[5]);
    const long long nskip = atoll(argv[6]);
    switch (n) {
      case 1: return print_run<1>(delay, forget, p0, nskip, T, argv + 7);
      case 2: return print_run<2>(delay, forget, p0, nskip, T, argv + 7);
      case 3: return print_run<3>(delay, forget, p0, nskip, T, argv + 7);
      case 4: return print_run<4>(delay, forget, p0, nskip, T, argv + 7);
      case 5: return print_run<5>(delay, forget, p0, nskip, T, argv + 7);
      case 6: return print_run<6>(delay, forget, p0, nskip, T, argv + 7);
      case 7: return print_run<7>(delay, forget, p0, nskip, T, argv + 7);
      case 8: return print_run<8>(delay, forget, p0, nskip, T, argv + 7);
    }
    fprintf(stderr, "order %d\n", n);
    return 2;
  }
  // ---- the update
  REQUIRE(run_all<1>() == 0 && run_all<2>() == 0 && run_all<3>() == 0 && run_all<4>() == 0);
  REQUIRE(run_all<5>() == 0 && run_all<6>() == 0 && run_all<7>() == 0 && run_all<8>() == 0);
  REQUIRE(PR_SLOTS(8) == 8 + 36 + 10 + 2 && PR_SLOTS(1) == 1 + 1 + 3 + 2 && PR_IJ(8, 7, 7) == 35 && PR_IJ(8, 1, 1) == 8);

  // ---- the counters: learned frames of a push of n frames at once == pushed one by one
  for (int order : {1, 4, 8})
    for (int n : {1, 3, 7, 50}) {
      PrCounts a, b;
      for (int rep = 0; rep < 4; rep++) {
        if (rep == 2) { a.since = 0; b.since = 0; }
        const bool learning = rep != 3;
        REQUIRE(pr_advance(a, n, order, learning) == b.since);
        for (int t = 0; t < n; t++) pr_advance(b, 1, order, learning);
        REQUIRE(a.total == b.total && a.since == b.since && a.learned == b.learned);
      }
    }

  // ---- the validators
  std::string err;
  aomarl_predictor_desc ok;
  ok.nenv = 3; ok.nmodes = 5; ok.order = 4; ok.nskip = 50; ok.delay = 1.f; ok.forget = 1.0; ok.p0 = 1e4;
  REQUIRE(pr_validate(&ok, err) == 0);
  REQUIRE(pr_validate(nullptr, err) == 1 && err.find("null desc") != std::string::npos);
  { auto d = ok; d.nenv = 0; REQUIRE(pr_validate(&d, err) == 1 && err.find("predictor_create: nenv") == 0); }
  { auto d = ok; d.nmodes = -1; REQUIRE(pr_validate(&d, err) == 1 && err.find("nmodes") != std::string::npos); }
  { auto d = ok; d.nenv = 70000; d.nmodes = 70000; REQUIRE(pr_validate(&d, err) == 1 && err.find("2^31") != std::string::npos); }
  for (int o : {0, -1, 9, 100}) { auto d = ok; d.order = o; REQUIRE(pr_validate(&d, err) == 1 && err.find("order") != std::string::npos); }
  for (int o = 1; o <= 8; o++) { auto d = ok; d.order = o; REQUIRE(pr_validate(&d, err) == 0); }
  { auto d = ok; d.nskip = -1; REQUIRE(pr_validate(&d, err) == 1 && err.find("nskip") != std::string::npos); }
  for (float dl : {-0.1f, 2.5f, NAN, INFINITY}) { auto d = ok; d.delay = dl; REQUIRE(pr_validate(&d, err) == 1 && err.find("delay") != std::string::npos); }
  for (float dl : {0.f, 0.4f, 2.f}) { auto d = ok; d.delay = dl; REQUIRE(pr_validate(&d, err) == 0); }
  for (double f : {0.0, -0.5, 1.0000001, (double)NAN, (double)INFINITY}) { auto d = ok; d.forget = f; REQUIRE(pr_validate(&d, err) == 1 && err.find("forget") != std::string::npos); }
  for (double f : {1e-6, 0.98, 1.0}) { auto d = ok; d.forget = f; REQUIRE(pr_validate(&d, err) == 0); }
  for (double v : {0.0, -1.0, (double)NAN, (double)INFINITY}) { auto d = ok; d.p0 = v; REQUIRE(pr_validate(&d, err) == 1 && err.find("p0") != std::string::npos); }

  { const int n = 3, ns = 2;
    std::vector<double> th(ns * n, 0.25), P(ns * n * n, 0.0);
    for (int s = 0; s < ns; s++) for (int i = 0; i < n; i++) { P[(s * n + i) * n + i] = 2.0 + i; }
    P[1] = P[3] = 0.5;
    REQUIRE(pr_validate_set(ns, n, th.data(), P.data(), err) == 0);
    REQUIRE(pr_validate_set(ns, n, nullptr, P.data(), err) == 0 && pr_validate_set(ns, n, th.data(), nullptr, err) == 0);
    REQUIRE(pr_validate_set(ns, n, nullptr, nullptr, err) == 0);
    { auto t = th; t[4] = NAN; REQUIRE(pr_validate_set(ns, n, t.data(), P.data(), err) == 1 && err.find("theta[4]") != std::string::npos); }
    { auto Q = P; Q[n * n + 2] = 0.1; REQUIRE(pr_validate_set(ns, n, th.data(), Q.data(), err) == 1 && err.find("series 1 is not symmetric") != std::string::npos); }
    { auto Q = P; Q[4] = 0.0; REQUIRE(pr_validate_set(ns, n, th.data(), Q.data(), err) == 1 && err.find("not positive") != std::string::npos); }
    { auto Q = P; Q[8] = -3.0; REQUIRE(pr_validate_set(ns, n, th.data(), Q.data(), err) == 1 && err.find("not positive") != std::string::npos); }
    { auto Q = P; Q[1] = Q[3] = INFINITY; REQUIRE(pr_validate_set(ns, n, th.data(), Q.data(), err) == 1 && err.find("non-finite") != std::string::npos); }
  }
  printf("predictor_host_check: ok\n");
  return 0;
}
