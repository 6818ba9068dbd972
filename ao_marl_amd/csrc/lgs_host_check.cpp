// lgs_host_check.cpp -- a stand-alone host program around the host half of the laser-guide-star sensor
// (aomarl_lgs_host.h: the validation of the desc, of the kernels and of the arguments of trace and measure, the kernel's
// table in the lag domain and the launch plan), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o lgs_host_check lgs_host_check.cpp
// No GPU, no HIP.  Exit status 0: all held.
#include "aomarl_lgs_host.h"

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main() {
  std::string err;
  // ---- the desc
  const int n = 40, pd = LGS_PD, N = LGS_N, nvalid = 4;
  std::vector<float> mp((size_t)n * n, 1.f), hxy((size_t)pd * pd, 0.f), flux(nvalid, 1.f);
  std::vector<int32_t> x0 = {2, 18, 2, 18}, y0 = {2, 2, 18, 24};
  aomarl_lgs_desc ok = {};
  ok.nenv = 3; ok.n = n; ok.pdiam = pd; ok.N = N; ok.npix = 16; ok.nrebin = 2; ok.nvalid = nvalid;
  ok.lambda_um = 0.5f; ok.nphotons = 1e4f; ok.noise = -1.f; ok.cog_offset = 7.5f; ok.cog_scale = 0.25f;
  ok.mpupil = mp.data(); ok.halfxy = hxy.data(); ok.flux = flux.data(); ok.sub_x0 = x0.data(); ok.sub_y0 = y0.data();
  REQUIRE(lgs_validate(&ok, err) == 0);
  REQUIRE(lgs_validate(nullptr, err) == 1 && has(err, "null desc"));
  for (int v : {8, 15, 32, 0, -16}) { auto d = ok; d.pdiam = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "built for pdiam = 16 with N = 64 and pdiam = 8 with N = 32")); }
  for (int v : {32, 128, 0}) { auto d = ok; d.N = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "built for")); }
  { auto d = ok; d.pdiam = LGS_PD_S; d.N = LGS_N_S; d.npix = 16; d.nrebin = 2; REQUIRE(lgs_validate(&d, err) == 0); }
  { auto d = ok; d.pdiam = LGS_PD_S; d.N = LGS_N_S; d.npix = 17; d.nrebin = 2; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "npix")); }
  for (int v : {0, 33, -1}) { auto d = ok; d.npix = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "npix")); }
  for (int v : {0, 5, -2}) { auto d = ok; d.nrebin = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "nrebin")); }
  { auto d = ok; d.npix = 32; d.nrebin = 2; REQUIRE(lgs_validate(&d, err) == 0); }
  for (int v : {0, 65536, -1}) { auto d = ok; d.nenv = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "nenv")); }
  for (int v : {0, 15, 40000}) { auto d = ok; d.n = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "n =")); }
  for (int v : {0, -3, 65536}) { auto d = ok; d.nvalid = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "nvalid")); }
  for (float v : {0.f, -1.f, NAN, INFINITY}) { auto d = ok; d.lambda_um = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "lambda_um")); }
  for (float v : {0.f, -5.f, NAN}) { auto d = ok; d.nphotons = v; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "nphotons")); }
  { auto d = ok; d.noise = NAN; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "noise")); }
  { auto d = ok; d.cog_scale = INFINITY; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "cog_offset / cog_scale")); }
  { auto d = ok; d.flux = nullptr; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "null array")); }
  { auto w = x0; w[1] = n - pd + 1; auto d = ok; d.sub_x0 = w.data(); REQUIRE(lgs_validate(&d, err) == 1 && has(err, "sub-aperture 1 lies outside")); }
  { auto w = y0; w[3] = -1; auto d = ok; d.sub_y0 = w.data(); REQUIRE(lgs_validate(&d, err) == 1 && has(err, "sub-aperture 3 lies outside")); }
  { auto w = y0; w[3] = n - pd; auto d = ok; d.sub_y0 = w.data(); REQUIRE(lgs_validate(&d, err) == 0); }
  { auto f = flux; f[2] = -0.5f; auto d = ok; d.flux = f.data(); REQUIRE(lgs_validate(&d, err) == 1 && has(err, "flux[2]")); }
  { auto d = ok; d.nenv = 40000; d.nvalid = 60000; REQUIRE(lgs_validate(&d, err) == 1 && has(err, "2^31")); }

  // ---- the kernels and their table
  std::vector<float> K((size_t)2 * N * N, 0.f);
  K[(size_t)(N / 2) * N + N / 2] = 1.f;                                      // kernel 0: the impulse at the centre
  for (int y = 0; y < N; y++)
    for (int x = 0; x < N; x++) {
      const double u = x - N / 2 - 0.3 * (y - N / 2), v = y - N / 2;
      K[(size_t)N * N + (size_t)y * N + x] = (float)exp(-(u * u / 18.0 + v * v / 8.0));
    }
  REQUIRE(lgs_validate_kernels(K.data(), 2, N, err) == 0);
  REQUIRE(lgs_validate_kernels(nullptr, 2, N, err) == 1 && has(err, "null array"));
  { auto b = K; b[5] = -1e-3f; REQUIRE(lgs_validate_kernels(b.data(), 2, N, err) == 1 && has(err, "kernel 0, pixel 5")); }
  { auto b = K; b[(size_t)N * N + 7] = NAN; REQUIRE(lgs_validate_kernels(b.data(), 2, N, err) == 1 && has(err, "kernel 1, pixel 7")); }
  { auto b = K; b[(size_t)(N / 2) * N + N / 2] = 0.f; REQUIRE(lgs_validate_kernels(b.data(), 2, N, err) == 1 && has(err, "kernel 0 sums to zero")); }
  const int L = pd - 1, per = (2 * L + 1) * pd;
  std::vector<float> tab((size_t)2 * per);
  lgs_kernel_table(K.data(), pd, N, tab.data());
  for (int sy = -L; sy <= L; sy++)
    for (int sx = 0; sx < pd; sx++) {                                         // the impulse: (-1)^(sy + sx)
      const float want = ((sy + sx) & 1) ? -1.f : 1.f;
      REQUIRE(fabsf(tab[2 * ((sy + L) * pd + sx)] - want) < 1e-6f && fabsf(tab[2 * ((sy + L) * pd + sx) + 1]) < 1e-6f);
    }
  lgs_kernel_table(K.data() + (size_t)N * N, pd, N, tab.data());
  {                                                                           // against the definition, a few lags
    const float *k1 = K.data() + (size_t)N * N;
    double sum = 0;
    for (int i = 0; i < N * N; i++) sum += k1[i];
    REQUIRE(fabs(tab[2 * (L * pd)] - sum) < 1e-4 * sum && fabsf(tab[2 * (L * pd) + 1]) < 1e-4 * sum);
    const int lags[3][2] = {{-15, 15}, {7, 3}, {-4, 0}};
    for (auto &g : lags) {
      std::complex<double> a = 0;
      for (int y = 0; y < N; y++)
        for (int x = 0; x < N; x++) a += (double)k1[(size_t)y * N + x] * std::polar(1.0, 2.0 * M_PI * (y * g[0] + x * g[1]) / N);
      const size_t o = 2 * ((size_t)(g[0] + L) * pd + g[1]);
      REQUIRE(fabs(tab[o] - a.real()) < 1e-5 * sum && fabs(tab[o + 1] - a.imag()) < 1e-5 * sum);
    }
    for (int sy = 1; sy <= L; sy++)                                           // Hermitian on the column sx = 0
      REQUIRE(fabsf(tab[2 * ((L + sy) * pd)] - tab[2 * ((L - sy) * pd)]) < 1e-4 * sum &&
              fabsf(tab[2 * ((L + sy) * pd) + 1] + tab[2 * ((L - sy) * pd) + 1]) < 1e-4 * sum);
  }

  // ---- trace
  const int known = 15;
  { float d[3] = {0.f, -0.05f, -0.1556f};
    REQUIRE(lgs_validate_trace(d, 3, 3, 8, 4, 0, 4, 7, known, err) == 0);
    REQUIRE(lgs_validate_trace(nullptr, 3, 3, 8, 4, 0, 4, 7, known, err) == 1 && has(err, "null dm1"));
    REQUIRE(lgs_validate_trace(d, 2, 3, 8, 4, 0, 4, 7, known, err) == 1 && has(err, "2 values for 3 layers"));
    REQUIRE(lgs_validate_trace(d, 3, 3, 8, 4, 2, 3, 7, known, err) == 1 && has(err, "environments"));
    REQUIRE(lgs_validate_trace(d, 3, 3, 8, 4, 0, 0, 7, known, err) == 1 && has(err, "environments"));
    REQUIRE(lgs_validate_trace(d, 3, 3, 8, 4, 0, 4, 16, known, err) == 1 && has(err, "unknown flags"));
    for (float v : {-1.f, -2.f, 0.1f, NAN}) { float b[3] = {0.f, v, 0.f}; REQUIRE(lgs_validate_trace(b, 3, 3, 8, 4, 0, 4, 7, known, err) == 1 && has(err, "dm1[1]")); } }

  // ---- measure
  REQUIRE(lgs_validate_measure(4, 0, 4, 0, false, false, -1.f, err) == 0);
  REQUIRE(lgs_validate_measure(4, 1, 3, AOMARL_LGS_NOISE | AOMARL_LGS_WRITE_CUBE, true, true, 0.5f, err) == 0);
  REQUIRE(lgs_validate_measure(4, 1, 4, 0, false, false, -1.f, err) == 1 && has(err, "environments"));
  REQUIRE(lgs_validate_measure(4, -1, 2, 0, false, false, -1.f, err) == 1 && has(err, "environments"));
  REQUIRE(lgs_validate_measure(4, 0, 4, 4, false, false, -1.f, err) == 1 && has(err, "unknown flags"));
  REQUIRE(lgs_validate_measure(4, 0, 4, AOMARL_LGS_NOISE, false, false, 0.f, err) == 1 && has(err, "without seeds"));
  REQUIRE(lgs_validate_measure(4, 0, 4, AOMARL_LGS_NOISE, false, false, -1.f, err) == 0);      // a noise-free sensor draws nothing
  REQUIRE(lgs_validate_measure(4, 0, 4, AOMARL_LGS_WRITE_CUBE, false, false, -1.f, err) == 1 && has(err, "without an image"));

  // ---- the plan: the window of the unrolled binmap lies inside the image, centred on pixel N / 2
  for (int N : {LGS_N, LGS_N_S})
  for (int npix = 1; npix <= LGS_NPIX_MAX; npix++)
    for (int nrebin = 1; npix * nrebin <= N; nrebin++) {
      const LgsPlan p = lgs_plan(1240, 256, npix, nrebin, N, (npix & 1) != 0);
      REQUIRE(p.window == npix * nrebin && p.indi >= 0 && p.indi + p.window <= N);
      REQUIRE(p.grid_x == 1240u && p.grid_y == 256u && p.threads == LGS_THREADS && p.launches == ((npix & 1) ? 2 : 1));
      if (p.window % 2 == 0) REQUIRE(p.indi + p.window / 2 == N / 2);
    }
  printf("lgs_host_check: ok\n");
  return 0;
}
