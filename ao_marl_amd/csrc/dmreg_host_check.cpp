// dmreg_host_check.cpp -- a stand-alone host program around the host half of the mirror mis-registration
// (aomarl_dmreg_host.h: the four-parameter form, the validation of table rows, ranges and of the context's state, the
// coordinate bound and the byte count), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o dmreg_host_check dmreg_host_check.cpp
// No GPU, no HIP.  Exit status 0: all held.
#include "aomarl_dmreg_host.h"
#include <vector>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main() {
  std::string err;
  const int nenv = 5, ndm = 2, dim = 104, nn = 88;
  // ---- create
  REQUIRE(dmreg_validate_create(nenv, ndm, err) == 0);
  for (int v : {0, -3, 65536}) REQUIRE(dmreg_validate_create(v, ndm, err) == 1 && has(err, "nenv"));
  REQUIRE(dmreg_validate_create(nenv, 0, err) == 1 && has(err, "mirrors"));
  REQUIRE(dmreg_validate_geometry(nn, 8.0, 8.0, dim, 0, err) == 0);
  REQUIRE(dmreg_validate_geometry(nn, 8.0, 8.0, 0, 1, err) == 1 && has(err, "mirror 1"));
  REQUIRE(dmreg_validate_geometry(nn, 1e12, 8.0, dim, 0, err) == 1 && has(err, "int32"));
  REQUIRE(dmreg_validate_geometry(nn, 8.0, NAN, dim, 0, err) == 1 && has(err, "int32"));
  REQUIRE(dmreg_validate_geometry(nn, 8.0, 8.0, 400000000, 0, err) == 1 && has(err, "int32"));
  // ---- the context's state
  REQUIRE(dmreg_validate_ctx(false, false, "dmreg_trace", err) == 0);
  REQUIRE(dmreg_validate_ctx(true, false, "dmreg_trace", err) == 1 && has(err, "pipelined frame") && has(err, "dmreg_trace"));
  REQUIRE(dmreg_validate_ctx(false, true, "dmreg_create", err) == 1 && has(err, "prefetched reset") && has(err, "dmreg_create"));
  // ---- ranges
  REQUIRE(dmreg_validate_range(nenv, ndm, 0, nenv, 1, "dmreg_set", err) == 0);
  REQUIRE(dmreg_validate_range(nenv, ndm, 4, 1, 0, "dmreg_set", err) == 0);
  for (int b : {-1, 5}) REQUIRE(dmreg_validate_range(nenv, ndm, b, 1, 0, "dmreg_set", err) == 1 && has(err, "environments"));
  for (int n : {0, -2, 6}) REQUIRE(dmreg_validate_range(nenv, ndm, 0, n, 0, "dmreg_set", err) == 1 && has(err, "environments"));
  REQUIRE(dmreg_validate_range(nenv, ndm, 3, 3, 0, "dmreg_get", err) == 1 && has(err, "dmreg_get"));
  REQUIRE(dmreg_validate_range(nenv, ndm, 2147483647, 2147483647, 0, "dmreg_set", err) == 1 && has(err, "environments"));
  for (int k : {-1, 2, 9}) REQUIRE(dmreg_validate_range(nenv, ndm, 0, 1, k, "dmreg_set", err) == 1 && has(err, "mirror"));
  REQUIRE(dmreg_validate_trace(nenv, 0, 0, 0, 7, 15, err) == 0);
  REQUIRE(dmreg_validate_trace(nenv, 1, 4, 1, 15, 15, err) == 0);
  REQUIRE(dmreg_validate_trace(nenv, 1, 5, 1, 7, 15, err) == 1 && has(err, "environments"));
  REQUIRE(dmreg_validate_trace(nenv, -1, 1, 1, 7, 15, err) == 1 && has(err, "environments"));
  for (int t : {-1, 2}) REQUIRE(dmreg_validate_trace(nenv, 0, 1, t, 7, 15, err) == 1 && has(err, "target"));
  REQUIRE(dmreg_validate_trace(nenv, 0, 1, 0, 16, 15, err) == 1 && has(err, "flags"));
  // ---- rows
  std::vector<float> rows(3 * DMREG_ROW);
  dmreg_identity(rows.data(), 3);
  for (int i = 0; i < 3; i++)
    REQUIRE(rows[6 * i] == 1.f && rows[6 * i + 1] == 0.f && rows[6 * i + 2] == 0.f && rows[6 * i + 3] == 1.f && rows[6 * i + 4] == 0.f && rows[6 * i + 5] == 0.f);
  REQUIRE(dmreg_validate_rows(rows.data(), 3, dim, err) == 0);
  REQUIRE(dmreg_validate_rows(nullptr, 3, dim, err) == 1 && has(err, "null"));
  for (int j = 0; j < DMREG_ROW; j++)
    for (float bad : {NAN, INFINITY, -INFINITY}) {
      auto r = rows; r[DMREG_ROW + j] = bad;
      REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 1 && has(err, "not finite") && has(err, "row 1"));
      REQUIRE(dmreg_validate_rows(r.data(), 1, dim, err) == 0);       // only the rows handed over are read
    }
  { auto r = rows; r[0] = 4.5f; r[3] = 0.5f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 1 && has(err, "exceeds")); }
  { auto r = rows; r[1] = -1e30f; r[2] = 1e-30f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 1 && has(err, "exceeds")); }
  { auto r = rows; r[0] = 0.4f; r[3] = 0.5f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 1 && has(err, "det A")); }
  { auto r = rows; r[0] = 2.5f; r[3] = 2.f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 1 && has(err, "det A")); }
  { auto r = rows; r[0] = 1.f; r[1] = 1.f; r[2] = 1.f; r[3] = 1.f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 1 && has(err, "det A")); }
  { auto r = rows; r[0] = 0.5f; r[3] = 0.5f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 0); }     // the ends are in
  { auto r = rows; r[0] = 2.f; r[3] = 2.f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 0); }
  { auto r = rows; r[0] = 0.f; r[1] = -1.f; r[2] = 1.f; r[3] = 0.f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 0); }   // quarter turn
  { auto r = rows; r[3] = -1.f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 0); }                  // a mirror image
  { auto r = rows; r[2 * DMREG_ROW + 4] = 4.f * dim + 1.f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 1 && has(err, "|t|") && has(err, "row 2")); }
  { auto r = rows; r[5] = -4.f * dim - 1.f; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 1 && has(err, "|t|")); }
  { auto r = rows; r[4] = 4.f * dim; r[5] = -4.f * dim; REQUIRE(dmreg_validate_rows(r.data(), 3, dim, err) == 0); }
  // ---- the four-parameter form: by hand for theta = 90 degrees, G = 2, shift (3, -1)
  float row[DMREG_ROW];
  dmreg_affine(3.0, -1.0, M_PI / 2, 2.0, row);
  REQUIRE(fabsf(row[0]) < 1e-7f && row[1] == 0.5f && row[2] == -0.5f && fabsf(row[3]) < 1e-7f);
  REQUIRE(fabsf(row[4] - 0.5f) < 1e-6f && fabsf(row[5] - 1.5f) < 1e-6f);     // t = -A (3, -1) = -(-0.5, -1.5)
  dmreg_affine(0.0, 0.0, 0.0, 1.0, row);
  REQUIRE(row[0] == 1.f && row[1] == 0.f && row[2] == 0.f && row[3] == 1.f && row[4] == 0.f && row[5] == 0.f);
  // whatever the four parameters inside the accepted magnifications, the row passes; outside it is refused by name
  for (double G : {0.55, 0.8, 1.0, 1.3, 1.9})
    for (double th : {-3.0, -0.02, 0.0, 0.001, 0.5, 1.5707963267948966})
      for (double sh : {-40.0, 0.0, 0.3, 17.25}) {
        dmreg_affine(sh, -0.5 * sh, th, G, row);
        REQUIRE(dmreg_validate_rows(row, 1, dim, err) == 0);
      }
  dmreg_affine(0.0, 0.0, 0.1, 0.45, row);
  REQUIRE(dmreg_validate_rows(row, 1, dim, err) == 1 && has(err, "det A"));
  dmreg_affine(0.0, 0.0, 0.1, 2.2, row);
  REQUIRE(dmreg_validate_rows(row, 1, dim, err) == 1 && has(err, "det A"));
  dmreg_affine(5.0 * dim, 0.0, 0.0, 1.0, row);
  REQUIRE(dmreg_validate_rows(row, 1, dim, err) == 1 && has(err, "|t|"));
  // ---- the sample position: the identity row is (x + ox, y + oy) exactly; the extreme accepted rows stay inside the
  // bound, and the bound inside what a float -> int conversion holds
  dmreg_identity(row, 1);
  for (int g : {88, 80, 648, 640})
    for (float off : {0.f, 8.f, 12.5f, -3.25f})
      for (int x : {0, 1, g / 2, g - 1}) {
        float u, v;
        dmreg_sample(row, g, off, -off, x, g - 1 - x, &u, &v);
        REQUIRE(u == (float)x + off && v == (float)(g - 1 - x) - off);
      }
  const double bound = dmreg_coord_bound(nn, 8.0, dim);
  REQUIRE(bound < DMREG_COORD_MAX && DMREG_COORD_MAX < 2147483647.0);
  for (float a : {-4.f, 4.f})
    for (float b : {-4.f, 4.f})
      for (float t : {-4.f * dim, 4.f * dim})
        for (int x : {0, nn - 1})
          for (int y : {0, nn - 1}) {
            const float ext[DMREG_ROW] = {a, b, b, a, t, -t};
            float u, v;
            dmreg_sample(ext, nn, 8.f, 8.f, x, y, &u, &v);
            REQUIRE(fabs((double)u) <= bound * (1 + 1e-6) && fabs((double)v) <= bound * (1 + 1e-6));
            const int iu = (int)floorf(u), iv = (int)floorf(v);     // defined: far inside int32
            REQUIRE((double)iu <= (double)u && (double)iv <= (double)v);
          }
  // ---- bytes of a trace from shapes
  const int dims[2] = {104, 104}, tt[2] = {0, 1};
  long long shared = 0;
  const long long bytes = dmreg_trace_bytes(nn, 3, 2, dims, tt, &shared);
  REQUIRE(bytes == 4LL * nn * nn * 3 + 4LL * nn * nn + 4LL * nn * nn + 8 && shared == 8LL * nn * nn);
  const int small[1] = {40};
  REQUIRE(dmreg_trace_bytes(nn, 0, 1, small, tt, nullptr) == 4LL * nn * nn + 4LL * 40 * 40);
  printf("dmreg_host_check: ok\n");
  return 0;
}
