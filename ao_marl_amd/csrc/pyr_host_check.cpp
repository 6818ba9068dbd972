// pyr_host_check.cpp -- a stand-alone host program around the host half of the pyramid sensor (aomarl_pyr_host.h: the
// validation of the desc, of the modulation and of a measure's arguments, the batch plan and the launch count), meant to
// be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o pyr_host_check pyr_host_check.cpp
// No GPU, no HIP.  Exit status 0: all held.
#include "aomarl_pyr_host.h"
#include <vector>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main() {
  std::string err;
  // ---- the desc
  const int n = 36, N = 128, nrebin = 4, nb = N / nrebin, nvalid = 5;
  std::vector<float> mp((size_t)n * n, 0.f), plane((size_t)N * N, 1.f);
  for (int y = 2; y < n - 2; y++) for (int x = 2; x < n - 2; x++) mp[(size_t)y * n + x] = 1.f;
  std::vector<int32_t> vx(4 * nvalid), vy(4 * nvalid);
  for (int i = 0; i < 4 * nvalid; i++) { vx[i] = i % nb; vy[i] = (3 * i) % nb; }
  aomarl_pyr_desc ok = {};
  ok.nenv = 3; ok.n = n; ok.Nfft = N; ok.nrebin = nrebin; ok.nvalid = nvalid; ok.npts_max = 16; ok.pixel_filter = 1;
  ok.lambda_um = 0.5f; ok.nphotons = 1e5f; ok.noise = -1.f; ok.thresh = 1e-4f;
  ok.mpupil = mp.data(); ok.halfxy = plane.data(); ok.submask = plane.data(); ok.sincar = plane.data();
  ok.validsubsx = vx.data(); ok.validsubsy = vy.data();
  REQUIRE(pyr_validate(&ok, err) == 0);
  REQUIRE(pyr_validate(nullptr, err) == 1 && has(err, "null desc"));
  for (int v : {0, 32, 96, 4096, -128}) { auto d = ok; d.Nfft = v; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "Nfft")); }
  for (int v : {0, 35, 130, -2}) { auto d = ok; d.n = v; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "n =")); }
  for (int v : {0, 3, 5, -4}) { auto d = ok; d.nrebin = v; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "nrebin")); }
  { auto d = ok; d.nenv = 0; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "nenv")); }
  { auto d = ok; d.nenv = 65536; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "nenv")); }
  { auto d = ok; d.nenv = 40000; d.Nfft = 2048; d.nrebin = 4; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "2^31")); }
  for (int v : {0, -1, PYR_MAX_PAIRS + 1}) { auto d = ok; d.npts_max = v; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "npts_max")); }
  for (int v : {0, -3, nb * nb}) { auto d = ok; d.nvalid = v; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "nvalid")); }
  for (float v : {0.f, -1.f, NAN, INFINITY}) { auto d = ok; d.lambda_um = v; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "lambda_um")); }
  for (float v : {0.f, -5.f, NAN}) { auto d = ok; d.nphotons = v; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "nphotons")); }
  { auto d = ok; d.batch_kib = -1; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "batch_kib")); }
  { auto d = ok; d.noise = NAN; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "noise")); }
  { auto d = ok; d.thresh = INFINITY; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "thresh")); }
  { auto d = ok; d.mpupil = nullptr; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "null array")); }
  { auto d = ok; d.sincar = nullptr; REQUIRE(pyr_validate(&d, err) == 1 && has(err, "null array")); }
  { auto d = ok; d.sincar = nullptr; d.pixel_filter = 0; REQUIRE(pyr_validate(&d, err) == 0); }
  { std::vector<float> dark((size_t)n * n, 0.f); auto d = ok; d.mpupil = dark.data(); REQUIRE(pyr_validate(&d, err) == 1 && has(err, "no lit pixel")); }
  { auto w = vx; w[7] = nb; auto d = ok; d.validsubsx = w.data(); REQUIRE(pyr_validate(&d, err) == 1 && has(err, "validsubs[7]")); }
  { auto w = vy; w[19] = -1; auto d = ok; d.validsubsy = w.data(); REQUIRE(pyr_validate(&d, err) == 1 && has(err, "validsubs[19]")); }

  // ---- the modulation
  { float cx[4] = {0.1f, 0.f, -0.1f, 0.f}, cy[4] = {0.f, 0.1f, 0.f, -0.1f}, w[4] = {1.f, 2.f, 0.f, 0.5f};
    double ws = 0;
    REQUIRE(pyr_validate_modulation(cx, cy, w, 4, 16, 0.15f, &ws, err) == 0 && ws == 3.5);
    REQUIRE(pyr_validate_modulation(nullptr, cy, w, 4, 16, 0.15f, &ws, err) == 1 && has(err, "null array"));
    REQUIRE(pyr_validate_modulation(cx, cy, w, 0, 16, 0.15f, &ws, err) == 1 && has(err, "npts"));
    REQUIRE(pyr_validate_modulation(cx, cy, w, 4, 3, 0.15f, &ws, err) == 1 && has(err, "npts"));
    REQUIRE(pyr_validate_modulation(cx, cy, w, 4, 16, 0.f, &ws, err) == 1 && has(err, "s_scale"));
    REQUIRE(pyr_validate_modulation(cx, cy, w, 4, 16, NAN, &ws, err) == 1 && has(err, "s_scale"));
    { float bad[4] = {0.f, NAN, 0.f, 0.f}; REQUIRE(pyr_validate_modulation(bad, cy, w, 4, 16, 1.f, &ws, err) == 1 && has(err, "point 1")); }
    { float bad[4] = {1.f, 1.f, -1.f, 1.f}; REQUIRE(pyr_validate_modulation(cx, cy, bad, 4, 16, 1.f, &ws, err) == 1 && has(err, "weight 2")); }
    { float zero[4] = {0.f, 0.f, 0.f, 0.f}; REQUIRE(pyr_validate_modulation(cx, cy, zero, 4, 16, 1.f, &ws, err) == 1 && has(err, "sum to zero")); }
  }

  // ---- a measure's arguments
  REQUIRE(pyr_validate_measure(3, 0, 3, 0, 1, false, -1.f, err) == 0);
  REQUIRE(pyr_validate_measure(3, 1, 2, AOMARL_PYR_NOISE, 3, true, 0.f, err) == 0);
  REQUIRE(pyr_validate_measure(3, 1, 3, 0, 1, false, -1.f, err) == 1 && has(err, "environments"));
  REQUIRE(pyr_validate_measure(3, -1, 1, 0, 1, false, -1.f, err) == 1 && has(err, "environments"));
  REQUIRE(pyr_validate_measure(3, 0, 0, 0, 1, false, -1.f, err) == 1 && has(err, "environments"));
  REQUIRE(pyr_validate_measure(3, 0x7fffffff, 2, 0, 1, false, -1.f, err) == 1);
  for (int m : {-1, 4}) REQUIRE(pyr_validate_measure(3, 0, 3, 0, m, false, -1.f, err) == 1 && has(err, "method"));
  REQUIRE(pyr_validate_measure(3, 0, 3, 2, 1, false, -1.f, err) == 1 && has(err, "flags"));
  REQUIRE(pyr_validate_measure(3, 0, 3, AOMARL_PYR_NOISE, 1, false, 0.f, err) == 1 && has(err, "seeds"));
  REQUIRE(pyr_validate_measure(3, 0, 3, AOMARL_PYR_NOISE, 1, false, -1.f, err) == 0);      // (no noise to draw)

  // ---- the plan: the planes of a batch fit the budget, every pair is covered once, whole environments or one
  struct Shape { int n, N, nenv, npts; };
  for (Shape s : {Shape{36, 128, 3, 4}, Shape{52, 256, 3, 5}, Shape{164, 512, 64, 16}, Shape{164, 512, 3, 16},
                  Shape{644, 2048, 8, 16}, Shape{644, 2048, 1, 1}, Shape{36, 64, 5000, 1024}}) {
    const PyrPlan p = pyr_plan(s.n, s.N, s.nenv, s.npts);
    REQUIRE(p.cap >= 1 && p.cap <= PYR_MAX_PAIRS && (long long)p.cap <= (long long)s.nenv * s.npts);
    REQUIRE(p.cw * (long long)s.N * 8 <= 65536 && s.N % p.cw == 0);
    REQUIRE(p.cap == 1 || (long long)p.cap * (p.t1_stride + p.t2_stride) * 8 <= PYR_BATCH_BYTES);
    REQUIRE(p.filt_env >= 1 && p.filt_env <= s.nenv);
    REQUIRE(p.filt_env == 1 || 2LL * p.filt_env * p.t2_stride * 8 <= PYR_BATCH_BYTES);
    for (int npts : {1, s.npts / 2 > 0 ? s.npts / 2 : 1, s.npts}) {
      int env_b, pts_b;
      pyr_batch(p, npts, &env_b, &pts_b);
      REQUIRE(env_b >= 1 && pts_b >= 1 && (long long)env_b * pts_b <= p.cap);
      REQUIRE(pts_b == npts || env_b == 1);
      for (int count : {1, s.nenv}) {
        long long pairs = 0, launches = 0;
        for (int e0 = 0; e0 < count; e0 += env_b) {
          const int ne = count - e0 < env_b ? count - e0 : env_b;
          for (int k0 = 0; k0 < npts; k0 += pts_b) {
            const int nk = npts - k0 < pts_b ? npts - k0 : pts_b;
            REQUIRE(ne * nk <= p.cap);
            pairs += (long long)ne * nk; launches += 3;
          }
        }
        REQUIRE(pairs == (long long)count * npts);
        REQUIRE(pyr_launch_count(p, count, npts, false) == launches + 2);
        REQUIRE(pyr_launch_count(p, count, npts, true) == launches + 2 + 4 * ((count + p.filt_env - 1) / p.filt_env));
      }
    }
  }
  { const PyrPlan p = pyr_plan(164, 512, 64, 16);       // the 10x10 system at nxsub 20: two environments of 16 points a batch
    int env_b, pts_b;
    pyr_batch(p, 16, &env_b, &pts_b);
    REQUIRE(p.cap == 36 && env_b == 2 && pts_b == 16 && p.cw == 8 && p.filt_env == 24); }
  { const PyrPlan p = pyr_plan(644, 2048, 8, 16);       // 40x40: two pairs a batch, the points of an environment in 8 batches
    int env_b, pts_b;
    pyr_batch(p, 16, &env_b, &pts_b);
    REQUIRE(p.cap == 2 && env_b == 1 && pts_b == 2 && p.cw == 4 && p.filt_env == 1); }
  { const PyrPlan p = pyr_plan(36, 128, 3, 4, 200 << 10);      // a budget of one pair: the points of an environment one by one
    int env_b, pts_b;
    pyr_batch(p, 4, &env_b, &pts_b);
    REQUIRE(p.cap == 1 && env_b == 1 && pts_b == 1 && p.filt_env == 1 && pyr_launch_count(p, 3, 4, true) == 3 * 12 + 4 * 3 + 2); }
  printf("pyr_host_check: ok\n");
  return 0;
}
