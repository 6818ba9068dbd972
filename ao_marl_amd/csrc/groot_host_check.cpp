// groot_host_check.cpp -- a stand-alone host program around aomarl_groot_host.h and aomarl_groot_fn.h (the desc
// validation, the tap-list builders and the scalar structure functions of aomarl_groot_*), meant to be built with the
// address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o groot_host_check groot_host_check.cpp
// No GPU, no HIP.  It tabulates Ij0 as starlord.tabulateIj0 does, checks the tap lists of the three models against the
// reference's own loops written out (four separation matrices; the npts^2 double loop; the twelve terms of dCmm), the
// scalar functions at r = 0, on both sides of each branch point and beyond the table's end, and feeds the validators
// every malformed desc they are written to refuse.  Exit status 0: all held.
#include "aomarl_groot_host.h"
#include <math.h>
#include <stdlib.h>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static std::vector<double> TX(GR_NTAB), TY(GR_NTAB);

static void tabulate() {
  const int n = GR_NTAB;
  const double dt = (GR_TMAX - GR_TMIN) / (n - 1), small = exp(-4.0);
  const double A = 0.75 * pow(small, 1. / 3) * (1 - small * small / 112.);
  std::vector<double> y((size_t)n);
  for (int i = 0; i < n; i++) {
    const double t = GR_TMIN + i * dt;
    TX[i] = exp(t);
    y[i] = exp(-t * (5. / 3.)) * (1 - j0(TX[i]));
  }
  double run = 0.0;
  TY[0] = A;
  for (int i = 1; i < n; i++) {
    run += y[i - 1] + (y[i] - y[i - 1]) / 2.;
    TY[i] = run * dt + A;
  }
}

static double F(int kind, double x, double y, double x0, double L0) {
  return gr_eval(kind, sqrt(x * x + y * y), x0, L0, TX.data(), TY.data());
}

static double tap_sum(const std::vector<GrTap> &taps, int b, int per, double rx, double ry) {
  double s = 0.0;
  for (int t = 0; t < per; t++) {
    const GrTap &q = taps[(size_t)b * per + t];
    s += q.w * F(q.kind, rx + q.ox, ry + q.oy, q.x0, q.L0);
  }
  return s;
}

static bool near(double a, double b, double scale) { return fabs(a - b) <= 1e-12 * scale; }

int main() {
  tabulate();
  std::string err;
  const double *tx = TX.data(), *ty = TY.data();
  // ---- the scalar functions
  REQUIRE(gr_dphi_highpass(0.0, 0.25, tx, ty) == 0.0 && gr_rodconan(0.0, 25.0) == 0.0 && gr_dphi_lowpass(0.0, 0.25, 25.0, tx, ty) == 0.0);
  REQUIRE(gr_ij0t83(0.0, tx, ty) == 0.0);
  { // series | table: the two branches meet at x = e^-3 (the table starts from the series' value at e^-4)
    const double lo = gr_ij0t83(GR_XSMALL * (1 - 1e-9), tx, ty), hi = gr_ij0t83(GR_XSMALL * (1 + 1e-9), tx, ty);
    REQUIRE(lo > 0 && hi > 0 && fabs(lo - hi) <= 1e-5 * hi);
    REQUIRE(lo == 0.75 * pow(GR_XSMALL * (1 - 1e-9), 1. / 3) * (1 - pow(GR_XSMALL * (1 - 1e-9), 2) / 112.));
  }
  { // inside the table: between its neighbours, equal to the entries at the abscissae
    for (int j : {0, 1, 714, 5000, GR_NTAB - 2}) {
      if (TX[j] < GR_XSMALL) continue;
      REQUIRE(gr_ij0t83(TX[j], tx, ty) == TY[j]);
      const double mid = gr_ij0t83(0.5 * (TX[j] + TX[j + 1]), tx, ty);
      REQUIRE(mid >= TY[j] && mid <= TY[j + 1] && near(mid, 0.5 * (TY[j] + TY[j + 1]), TY[j + 1]));
    }
    // the table's end and beyond: clamped to the last entry
    REQUIRE(gr_ij0t83(TX[GR_NTAB - 1], tx, ty) == TY[GR_NTAB - 1]);
    REQUIRE(gr_ij0t83(TX[GR_NTAB - 1] * 1.5, tx, ty) == TY[GR_NTAB - 1] && gr_ij0t83(1e300, tx, ty) == TY[GR_NTAB - 1]);
    REQUIRE(fabs(TY[GR_NTAB - 1] - 1.1183343328701949) < 1e-3);          // the integral's limit, which dphi_highpass subtracts
  }
  { // rodconan: series | asymptotic form at 2 pi r / L0 = 4.71239
    const double L0 = 25.0, rb = GR_DPRF0 * L0 / (2 * M_PI);
    const double lo = gr_rodconan(rb * (1 - 1e-9), L0), hi = gr_rodconan(rb * (1 + 1e-9), L0);
    REQUIRE((2 * M_PI / L0) * rb * (1 - 1e-9) <= GR_DPRF0 && (2 * M_PI / L0) * rb * (1 + 1e-9) > GR_DPRF0);
    REQUIRE(lo > 0 && hi > 0 && fabs(lo - hi) <= 1e-4 * hi);
    REQUIRE(lo == -gr_macdo((2 * M_PI / L0) * rb * (1 - 1e-9)) * (0.1716613621245709486 * pow(L0, 5. / 3.)));
    REQUIRE(hi == gr_asymp_macdo((2 * M_PI / L0) * rb * (1 + 1e-9)) * (0.1716613621245709486 * pow(L0, 5. / 3.)));
    // Kolmogorov's 6.88 r^(5/3) at r << L0, up to the outer scale's first correction, 0.8 (2 pi r / L0)^(1/3) = 1.5 %
    REQUIRE(fabs(gr_rodconan(0.1, 1e5) / (6.88388 * pow(0.1, 5. / 3.)) - 1) < 3e-2);
    // low + high = rodconan
    REQUIRE(near(gr_dphi_lowpass(0.7, 0.25, L0, tx, ty) + gr_dphi_highpass(0.7, 0.25, tx, ty), gr_rodconan(0.7, L0), 10.0));
  }
  // ---- the tap lists against the reference's loops
  const double probes[][2] = {{0.0, 0.0}, {0.25, 0.0}, {-0.5, 0.75}, {1.25, -1.0}, {-1.75, -1.5}, {2.0, 2.0}};
  { // Cerr, two entries of three layers
    const int B = 2, L = 3;
    const double w[B * L] = {0.3, 0.5, 0.2, 0.11, 0.7, 0.19}, sx[B * L] = {0.01, -0.2, 0.4, 0.0, 0.3, -0.05},
                 sy[B * L] = {0.02, 0.1, -0.3, 0.0, 0.25, 0.6}, L0[B * L] = {2.0, 1e5, 25.0, 30.0, 1.0, 100.0};
    // what the reference builds per layer: vdt u(theta) and Htheta u(angleht) separately
    const double vx[B * L] = {0.004, -0.15, 0.1, 0.0, 0.1, -0.02}, vy[B * L] = {0.015, 0.04, -0.1, 0.0, 0.2, 0.5};
    aomarl_groot_form_desc f = {AOMARL_GROOT_CERR, B, L, 0, 0.25, w, sx, sy, L0};
    REQUIRE(gr_validate_form(&f, 45, 48, 45 * 48, 64, 4, err) == 0 && gr_taps_per_entry(&f) == 9);
    std::vector<GrTap> taps;
    gr_build_taps(&f, taps);
    REQUIRE(taps.size() == (size_t)B * 9);
    for (int b = 0; b < B; b++)
      for (auto &p : probes) {
        double want = 0.0, mag = 0.0;
        for (int l = 0; l < L; l++) {
          const int k = b * L + l;
          const double hx = sx[k] - vx[k], hy = sy[k] - vy[k];
          // C[i][j] and C[j][i] (the separation negated) of Ccov, Caniso and Cbp (:172-181)
          for (int sgn = 1; sgn >= -1; sgn -= 2) {
            const double x = sgn * p[0], y = sgn * p[1];
            const double M = F(0, x, y, 0.25, L0[k]), Mv = F(0, x - vx[k], y - vy[k], 0.25, L0[k]),
                         Mh = F(0, x - hx, y - hy, 0.25, L0[k]), Mhv = F(0, x - vx[k] - hx, y - vy[k] - hy, 0.25, L0[k]);
            want += (0.5 * (Mhv - Mh - Mv + M) + 0.5 * (Mh - M) + 0.5 * (Mv - M)) * w[k];
            mag += (fabs(Mhv) + fabs(M)) * fabs(w[k]);
          }
        }
        REQUIRE(near(tap_sum(taps, b, 9, p[0], p[1]), want, mag));
      }
  }
  for (int npts : {1, 3, 5}) {   // Calias: the npts^2 double loop (:594-599)
    const double d = 0.25, w[2] = {1.7, 0.4};
    std::vector<double> c((size_t)npts, 1.0);
    for (int i = 1; i < npts; i += 2) c[i] = 4.0;
    for (int i = 2; i < npts - 1; i += 2) c[i] = 2.0;
    const double h = npts > 1 ? d / (npts - 1) : 1.0;
    for (int model : {AOMARL_GROOT_CALIAS_XX, AOMARL_GROOT_CALIAS_YY}) {
      aomarl_groot_form_desc f = {model, 2, 1, npts, d, w, nullptr, nullptr, nullptr};
      REQUIRE(gr_validate_form(&f, 24, 48, 48 * 48, 64, 4, err) == 0);
      const int per = gr_taps_per_entry(&f);
      REQUIRE(per == 3 * (2 * npts - 1));
      std::vector<GrTap> taps;
      gr_build_taps(&f, taps);
      REQUIRE(taps.size() == (size_t)2 * per);
      for (int b = 0; b < 2; b++)
        for (auto &p : probes) {
          double want = 0.0, mag = 0.0;
          for (int k = 0; k < npts; k++)
            for (int q = 0; q < npts; q++) {
              const double o = (k - q) * h;
              const double e = model == AOMARL_GROOT_CALIAS_XX
                                   ? F(1, p[0] - d, p[1] + o, d, 1) + F(1, p[0] + d, p[1] + o, d, 1) - 2 * F(1, p[0], p[1] + o, d, 1)
                                   : F(1, p[0] + o, p[1] - d, d, 1) + F(1, p[0] + o, p[1] + d, d, 1) - 2 * F(1, p[0] + o, p[1], d, 1);
              want += e * c[k] * c[q];
              mag += 4 * fabs(F(1, p[0] + d, p[1] + d, d, 1)) * c[k] * c[q];
            }
          REQUIRE(near(tap_sum(taps, b, per, p[0], p[1]), want * w[b], mag * w[b] + 1e-3));
        }
    }
  }
  { // dCmm: the twelve terms of compute_dCmm_element (:862-890)
    const int L = 2;
    const double d = 0.5, w[L] = {0.6, 0.4}, vx[L] = {0.01, -0.008}, vy[L] = {0.0, 0.004}, L0[L] = {1.5, 1e5};
    for (int model : {AOMARL_GROOT_DCMM_XX, AOMARL_GROOT_DCMM_YY}) {
      aomarl_groot_form_desc f = {model, 1, L, 0, d, w, vx, vy, L0};
      REQUIRE(gr_validate_form(&f, 24, 24, 0, 64, 4, err) == 0 && gr_taps_per_entry(&f) == 12);
      std::vector<GrTap> taps;
      gr_build_taps(&f, taps);
      const double ex = model == AOMARL_GROOT_DCMM_XX ? d : 0.0, ey = d - ex;
      for (auto &p : probes) {
        double want = 0.0, mag = 0.0;
        for (int l = 0; l < L; l++) {
          const double x = p[0], y = p[1];
          double e = F(2, -x - ex + vx[l], -y - ey + vy[l], d, L0[l]) + F(2, -x + ex + vx[l], -y + ey + vy[l], d, L0[l]) -
                     2 * F(2, -x + vx[l], -y + vy[l], d, L0[l]);
          e -= F(2, x - ex + vx[l], y - ey + vy[l], d, L0[l]) + F(2, x + ex + vx[l], y + ey + vy[l], d, L0[l]) -
               2 * F(2, x + vx[l], y + vy[l], d, L0[l]);
          want += w[l] * 0.25 * e;
          mag += w[l] * 2 * fabs(F(2, x + ex, y + ey, d, L0[l]));
        }
        REQUIRE(near(tap_sum(taps, 0, 12, p[0], p[1]), want, mag + 1e-3));
      }
    }
  }
  // ---- every refusal, by the argument it names
  {
    aomarl_groot_desc d = {64, 4, 32, 128, tx, ty};
    REQUIRE(gr_validate_create(&d, err) == 0);
    REQUIRE(gr_validate_create(nullptr, err) == 1);
    { aomarl_groot_desc e = d; e.n_max = 0; REQUIRE(gr_validate_create(&e, err) == 1 && err.find("n_max = 0") != std::string::npos); }
    { aomarl_groot_desc e = d; e.n_max = GR_MAX_POINTS + 1; REQUIRE(gr_validate_create(&e, err) == 1 && err.find("n_max") != std::string::npos); }
    { aomarl_groot_desc e = d; e.batch_max = 0; REQUIRE(gr_validate_create(&e, err) == 1 && err.find("batch_max = 0") != std::string::npos); }
    { aomarl_groot_desc e = d; e.k_max = 0; REQUIRE(gr_validate_create(&e, err) == 1 && err.find("k_max = 0") != std::string::npos); }
    { aomarl_groot_desc e = d; e.m_max = -1; REQUIRE(gr_validate_create(&e, err) == 1 && err.find("m_max = -1") != std::string::npos); }
    { aomarl_groot_desc e = d; e.m_max = e.k_max = 0; REQUIRE(gr_validate_create(&e, err) == 0); }
    { aomarl_groot_desc e = d; e.taby = nullptr; REQUIRE(gr_validate_create(&e, err) == 1 && err.find("null tabx") != std::string::npos); }
    { std::vector<double> x = TX; x[7] = x[6]; aomarl_groot_desc e = d; e.tabx = x.data();
      REQUIRE(gr_validate_create(&e, err) == 1 && err.find("tabx[7]") != std::string::npos); }
    { std::vector<double> y = TY; y[9] = NAN; aomarl_groot_desc e = d; e.taby = y.data();
      REQUIRE(gr_validate_create(&e, err) == 1 && err.find("taby[9]") != std::string::npos); }
    const double one[2] = {1.0, 1.0}, bad[2] = {1.0, 0.0};
    aomarl_groot_form_desc f = {AOMARL_GROOT_CERR, 1, 2, 0, 0.25, one, one, one, one};
    REQUIRE(gr_validate_form(&f, 45, 45, 0, 64, 4, err) == 0);
    REQUIRE(gr_validate_form(nullptr, 45, 45, 0, 64, 4, err) == 1);
    { auto e = f; e.model = 5; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("model = 5") != std::string::npos); }
    { auto e = f; e.batch = 5; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("batch = 5") != std::string::npos); }
    { auto e = f; e.batch = 0; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("batch = 0") != std::string::npos); }
    REQUIRE(gr_validate_form(&f, 65, 65, 0, 64, 4, err) == 1 && err.find("n = 65") != std::string::npos);
    REQUIRE(gr_validate_form(&f, 0, 45, 0, 64, 4, err) == 1 && err.find("n = 0") != std::string::npos);
    REQUIRE(gr_validate_form(&f, 45, 44, 0, 64, 4, err) == 1 && err.find("ldo = 44") != std::string::npos);
    { auto e = f; e.batch = 2; e.nlayers = 1; REQUIRE(gr_validate_form(&e, 45, 48, 44 * 48 + 44, 64, 4, err) == 1 && err.find("stride_o") != std::string::npos);
      REQUIRE(gr_validate_form(&e, 45, 48, 44 * 48 + 45, 64, 4, err) == 0); }
    { auto e = f; e.nlayers = 0; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("nlayers = 0") != std::string::npos); }
    { auto e = f; e.nlayers = GR_MAX_LAYERS + 1; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("nlayers") != std::string::npos); }
    { auto e = f; e.x0 = 0.0; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("x0") != std::string::npos); }
    { auto e = f; e.w = nullptr; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("null w") != std::string::npos); }
    { auto e = f; e.sy = nullptr; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("null sx") != std::string::npos); }
    { auto e = f; e.L0 = bad; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("L0[1]") != std::string::npos); }
    const double nan2[2] = {1.0, NAN}, inf2[2] = {INFINITY, 1.0};
    { auto e = f; e.w = nan2; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("w[1] is not finite") != std::string::npos); }
    { auto e = f; e.sx = inf2; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("sx / sy[0]") != std::string::npos); }
    { auto e = f; e.sy = nan2; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("sx / sy[1]") != std::string::npos); }
    { auto e = f; e.L0 = inf2; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("L0[0]") != std::string::npos); }
    { auto e = f; e.x0 = INFINITY; REQUIRE(gr_validate_form(&e, 45, 45, 0, 64, 4, err) == 1 && err.find("x0") != std::string::npos); }
    { aomarl_groot_form_desc e = {AOMARL_GROOT_CALIAS_XX, 2, 1, 3, 0.25, nan2, nullptr, nullptr, nullptr};
      REQUIRE(gr_validate_form(&e, 24, 48, 48 * 48, 64, 4, err) == 1 && err.find("w[1] is not finite") != std::string::npos); }
    for (int npts : {0, 2, 4, GR_MAX_NPTS + 2}) {
      aomarl_groot_form_desc e = {AOMARL_GROOT_CALIAS_XX, 1, 1, npts, 0.25, one, nullptr, nullptr, nullptr};
      REQUIRE(gr_validate_form(&e, 24, 24, 0, 64, 4, err) == 1 && err.find("npts = ") != std::string::npos);
    }
    { aomarl_groot_form_desc e = {AOMARL_GROOT_CALIAS_YY, 1, 2, 3, 0.25, one, nullptr, nullptr, nullptr};
      REQUIRE(gr_validate_form(&e, 24, 24, 0, 64, 4, err) == 1 && err.find("nlayers = 2") != std::string::npos); }
    alignas(16) static float buf[8];
    REQUIRE(gr_validate_sandwich(30, 46, 48, 48, 30, buf, buf, buf, 32, 128, err) == 0);
    REQUIRE(gr_validate_sandwich(30, 46, 48, 48, 30, buf, buf, buf, 0, 0, err) == 1 && err.find("without a sandwich") != std::string::npos);
    REQUIRE(gr_validate_sandwich(33, 46, 48, 48, 33, buf, buf, buf, 32, 128, err) == 1 && err.find("m = 33") != std::string::npos);
    REQUIRE(gr_validate_sandwich(30, 129, 132, 132, 30, buf, buf, buf, 32, 128, err) == 1 && err.find("n = 129") != std::string::npos);
    REQUIRE(gr_validate_sandwich(30, 46, 48, 48, 30, nullptr, buf, buf, 32, 128, err) == 1 && err.find("null operand") != std::string::npos);
    REQUIRE(gr_validate_sandwich(30, 46, 46, 48, 30, buf, buf, buf, 32, 128, err) == 1 && err.find("ldg = 46") != std::string::npos);
    REQUIRE(gr_validate_sandwich(30, 46, 48, 44, 30, buf, buf, buf, 32, 128, err) == 1 && err.find("ldc = 44") != std::string::npos);
    REQUIRE(gr_validate_sandwich(30, 46, 48, 48, 30, buf + 1, buf, buf, 32, 128, err) == 1 && err.find("ldg") != std::string::npos);
    REQUIRE(gr_validate_sandwich(30, 46, 48, 48, 30, buf, buf + 2, buf, 32, 128, err) == 1 && err.find("ldc") != std::string::npos);
    REQUIRE(gr_validate_sandwich(30, 46, 48, 48, 29, buf, buf, buf, 32, 128, err) == 1 && err.find("ldo = 29") != std::string::npos);
  }
  printf("groot_host_check: ok\n");
  return 0;
}
