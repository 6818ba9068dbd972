// tomo_host_check.cpp -- a stand-alone host program around the host half of laser tomography (aomarl_tomo_host.h: the
// validation of the arguments of aomarl_tomo_trace and aomarl_tomo_cov, the (star, layer) tables and the covariance's
// scalar text), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o tomo_host_check tomo_host_check.cpp
// No GPU, no HIP.  Exit status 0: all held.
#include "aomarl_tomo_host.h"

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

// the covariance of one pair written as plain loops over layers and signs, from the definition: its own structure
// function call per tap, its own footprints
static int n_series = 0, n_asymptotic = 0;      // taps of the restatement on either branch of rodconan
static double restated(const aomarl_tomo_cov_desc &d, int a, int ea, int i, int b, int eb, int j, double *mag) {
  const double kap = 1e-6 * 206265.0 / d.d, um = 0.5 / (2.0 * M_PI), rad = 2.0 * M_PI / 1296000.0;
  double acc = 0.0;
  *mag = 0.0;
  for (int l = 0; l < d.nlayers; l++) {
    const double alt = d.layers[3 * l], r0 = d.layers[3 * l + 1], L0 = d.layers[3 * l + 2];
    const double w = kap * kap * pow(r0, -5.0 / 3.0) * um * um;
    const double da = 1.0 - alt / d.row_stars[3 * a + 2], db = 1.0 - alt / d.col_stars[3 * b + 2];
    const double uax = da * d.row_px[i] + alt * rad * d.row_stars[3 * a], uay = da * d.row_py[i] + alt * rad * d.row_stars[3 * a + 1];
    const double ubx = db * d.col_px[j] + alt * rad * d.col_stars[3 * b], uby = db * d.col_py[j] + alt * rad * d.col_stars[3 * b + 1];
    for (int s1 = 1; s1 >= -1; s1 -= 2)
      for (int s2 = 1; s2 >= -1; s2 -= 2) {
        double x = uax - ubx, y = uay - uby;
        if (ea == 0) x += s1 * da * d.d / 2; else y += s1 * da * d.d / 2;
        if (eb == 0) x -= s2 * db * d.d / 2; else y -= s2 * db * d.d / 2;
        (2 * M_PI * hypot(x, y) / L0 > GR_DPRF0 ? n_asymptotic : n_series)++;
        const double t = w * gr_rodconan(hypot(x, y), L0) / 2;
        acc += -(double)(s1 * s2) * t;
        *mag += fabs(t);
      }
  }
  return acc;
}

int main() {
  std::string err;
  // ---- the trace
  const int n = 168, nl = 3, K = 2, known = 15;
  int dims[8] = {172, 184, 210, 0, 0, 0, 0, 0};
  std::vector<float> off = {2.f, 2.f, 8.f, 8.f, 21.f, 21.f, 2.f, 2.f, 14.f, 8.f, 39.f, 21.f};
  std::vector<float> dm1 = {0.f, -0.05f, -0.1556f, 0.f, 0.f, 0.f};
  float planes[1];
  aomarl_tomo_desc ok = {K, nl, off.data(), dm1.data()};
  REQUIRE(tomo_validate_trace(&ok, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 0);
  REQUIRE(tomo_validate_trace(nullptr, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "null desc"));
  REQUIRE(tomo_validate_trace(&ok, nullptr, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "null planes"));
  for (int v : {0, 9, -1}) { auto d = ok; d.nstars = v; REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "stars: 1..8")); }
  { auto d = ok; d.nlayers = 2; REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "offsets for 2 layers, the context has 3")); }
  { auto d = ok; d.off = nullptr; REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "null off / dm1")); }
  { auto d = ok; d.dm1 = nullptr; REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "null off / dm1")); }
  REQUIRE(tomo_validate_trace(&ok, planes, nl, dims, n, 4, 2, 3, 7, known, err) == 1 && has(err, "environments"));
  REQUIRE(tomo_validate_trace(&ok, planes, nl, dims, n, 4, -1, 2, 7, known, err) == 1 && has(err, "environments"));
  REQUIRE(tomo_validate_trace(&ok, planes, nl, dims, n, 4, 0, 0, 7, known, err) == 1 && has(err, "environments"));
  REQUIRE(tomo_validate_trace(&ok, planes, nl, dims, n, 4, 0, 4, 16, known, err) == 1 && has(err, "unknown flags"));
  REQUIRE(tomo_validate_trace(&ok, planes, nl, dims, n, 40000, 0, 4, 7, known, err) == 1 && has(err, "2^31"));
  for (float v : {NAN, INFINITY}) { auto o = off; o[7] = v; auto d = ok; d.off = o.data(); REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "off of star 1, layer 0 is not finite")); }
  for (float v : {-1.f, -2.f, 0.1f, NAN}) { auto m = dm1; m[4] = v; auto d = ok; d.dm1 = m.data(); REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "dm1 of star 1, layer 1")); }
  { auto o = off; o[10] = 43.5f; auto d = ok; d.off = o.data();      // 167 + 43.5 > 209
    REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "footprint of star 1 leaves screen 2")); }
  { auto o = off; o[10] = 42.f; auto d = ok; d.off = o.data(); REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 0); }
  { auto o = off; o[3] = -14.f; auto d = ok; d.off = o.data();       // star 0, layer 1, y: 0 - 14 + 0.05 * 83.5 < 0
    REQUIRE(tomo_validate_trace(&d, planes, nl, dims, n, 4, 0, 4, 7, known, err) == 1 && has(err, "footprint of star 0 leaves screen 1")); }

  // ---- the covariance: validation
  const int na = 7, nb = 5;
  std::vector<double> ax(na), ay(na), bx(nb), by(nb);
  for (int i = 0; i < na; i++) { ax[i] = 0.37 * i - 1.1; ay[i] = 0.9 - 0.23 * i * i / 3.0; }
  for (int j = 0; j < nb; j++) { bx[j] = -0.8 + 0.41 * j; by[j] = 0.13 * j * j - 0.5; }
  std::vector<double> sa = {0., 0., INFINITY, 20., 0., 90e3, -10., 15., 60e3}, sb = {0., 0., INFINITY, 0., -20., 90e3};
  std::vector<double> lay = {0., 0.2, 25., 4500., 0.37, 1e5, 14000., 0.5, 2.};
  aomarl_tomo_cov_desc cd = {};
  cd.n_row = na; cd.n_col = nb; cd.k_row = 3; cd.k_col = 2; cd.nlayers = 3; cd.d = 0.2;
  cd.row_px = ax.data(); cd.row_py = ay.data(); cd.col_px = bx.data(); cd.col_py = by.data();
  cd.row_stars = sa.data(); cd.col_stars = sb.data(); cd.layers = lay.data();
  double o1[1];
  REQUIRE(tomo_validate_cov(&cd, o1, err) == 0);
  REQUIRE(tomo_validate_cov(nullptr, o1, err) == 1 && has(err, "null desc"));
  REQUIRE(tomo_validate_cov(&cd, nullptr, err) == 1 && has(err, "null out"));
  for (int v : {0, 9}) { auto d = cd; d.k_col = v; REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "column stars: 1..8")); }
  for (int v : {0, 9}) { auto d = cd; d.nlayers = v; REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "layers: 1..8")); }
  { auto d = cd; d.n_row = 0; REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "row points")); }
  for (double v : {0.0, -1.0, (double)NAN}) { auto d = cd; d.d = v; REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "d =")); }
  { auto d = cd; d.col_py = nullptr; REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "null array")); }
  { auto l2 = lay; l2[4] = 0.; auto d = cd; d.layers = l2.data(); REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "layer 1")); }
  { auto s2 = sa; s2[8] = 14000.; auto d = cd; d.row_stars = s2.data(); REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "star 2: gsalt = 14000 m is not above the highest layer")); }
  { auto s2 = sb; s2[3] = NAN; auto d = cd; d.col_stars = s2.data(); REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "direction is not finite")); }
  { auto p2 = bx; p2[2] = INFINITY; auto d = cd; d.col_px = p2.data(); REQUIRE(tomo_validate_cov(&d, o1, err) == 1 && has(err, "point 2 is not finite")); }

  // ---- the covariance: the scalar text against the restatement, every (star, axis) pair, both branches of rodconan
  std::vector<TomoStarLayer> rows, cols;
  std::vector<TomoLayer> tl;
  tomo_cov_tables(&cd, rows, cols, tl);
  REQUIRE(rows.size() == 9 && cols.size() == 6 && tl.size() == 3);
  REQUIRE(rows[0].delta == 1.0 && rows[2].delta == 1.0 && rows[2].sx == 0.0);          // the natural star
  REQUIRE(fabs(rows[3 + 2].delta - (1.0 - 14000.0 / 90e3)) < 1e-15);
  double worst = 0.0;
  for (int a = 0; a < 3; a++) for (int ea = 0; ea < 2; ea++) for (int i = 0; i < na; i++)
    for (int b = 0; b < 2; b++) for (int eb = 0; eb < 2; eb++) for (int j = 0; j < nb; j++) {
      double mag;
      const double want = restated(cd, a, ea, i, b, eb, j, &mag);
      const double got = tomo_cov_entry(ax[i], ay[i], rows.data() + a * 3, ea, bx[j], by[j], cols.data() + b * 3, eb, tl.data(), 3, cd.d);
      REQUIRE(isfinite(got) && mag > 0);
      const double e = fabs(got - want) / mag;
      worst = e > worst ? e : worst;
    }
  REQUIRE(worst <= 1e-12);
  REQUIRE(n_series > 1000 && n_asymptotic > 1000);      // (layer 2 has L0 = 2 m: separations on either side of 1.5 m)
  // the diagonal: kappa^2 sum_l D_l(delta_al d) / d^2; symmetric in (a, i, e) <-> (b, j, e') on the same points and stars
  {
    auto d = cd; d.col_px = ax.data(); d.col_py = ay.data(); d.n_col = na; d.col_stars = sa.data(); d.k_col = 3;
    tomo_cov_tables(&d, rows, cols, tl);
    for (int a = 0; a < 3; a++) {
      double diag = 0;
      for (int l = 0; l < 3; l++) diag += tl[l].w * gr_rodconan(rows[a * 3 + l].delta * d.d, tl[l].L0);
      for (int e = 0; e < 2; e++) {
        const double got = tomo_cov_entry(ax[2], ay[2], rows.data() + a * 3, e, ax[2], ay[2], cols.data() + a * 3, e, tl.data(), 3, d.d);
        REQUIRE(fabs(got - diag) <= 1e-12 * diag && diag > 0);
      }
    }
    const double x = tomo_cov_entry(ax[1], ay[1], rows.data() + 3, 0, ax[4], ay[4], cols.data() + 6, 1, tl.data(), 3, d.d);
    const double y = tomo_cov_entry(ax[4], ay[4], rows.data() + 6, 1, ax[1], ay[1], cols.data() + 3, 0, tl.data(), 3, d.d);
    REQUIRE(fabs(x - y) <= 1e-12 * (fabs(x) + 1e-30) + 1e-18);
  }
  printf("tomo_host_check: ok\n");
  return 0;
}
