// psfrec_host_check.cpp -- a stand-alone host program around aomarl_psfrec_host.h (the desc validation and the tap-list
// builder of aomarl_psfrec_create), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o psfrec_host_check psfrec_host_check.cpp
// No GPU, no HIP.  It builds a small pupil with Gaussian influence functions, checks the tap list against a dense
// product, and feeds the validator every malformed desc it is written to refuse.  Exit status 0: all held.
#include "aomarl_psfrec_host.h"
#include <math.h>
#include <stdlib.h>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

struct Sys {
  int p, N, nact;
  std::vector<int32_t> lit, indices, indptr;
  std::vector<float> data, tt, map;
  aomarl_psfrec_desc d;
};

static void make(Sys &s, int p, int N, int side, double radius) {
  s.p = p; s.N = N; s.nact = side * side;
  s.lit.clear(); s.indices.clear(); s.indptr.assign(1, 0); s.data.clear();
  const double c = 0.5 * (p - 1);
  for (int y = 0; y < p; y++)
    for (int x = 0; x < p; x++)
      if (hypot(x - c, y - c) <= 0.5 * p) s.lit.push_back(y * p + x);
  const int npts = (int)s.lit.size();
  for (int a = 0; a < s.nact; a++) {
    const double ay = (a / side + 0.5) * p / side, ax = (a % side + 0.5) * p / side;
    for (int i = 0; i < npts; i++) {
      const double r = hypot(s.lit[i] % p - ax, s.lit[i] / p - ay);
      if (r <= radius) { s.indices.push_back(i); s.data.push_back((float)exp(-r * r / (radius * radius))); }
    }
    s.indptr.push_back((int32_t)s.indices.size());
  }
  s.tt.assign(2 * (size_t)npts, 0.5f);
  s.map.assign((size_t)N * N, 1.f);
  s.d.p = p; s.d.N = N; s.d.npts = npts; s.d.nactu = s.nact + 2; s.d.ld_actu = s.nact + 2;
  s.d.lit = s.lit.data(); s.d.if_data = s.data.data(); s.d.if_indices = s.indices.data(); s.d.if_indptr = s.indptr.data();
  s.d.tt = s.tt.data(); s.d.denmask = s.d.mask = s.d.otftel = s.map.data();
}

int main() {
  std::string err;
  Sys s;
  make(s, 33, 128, 6, 9.0);
  REQUIRE(pr_validate(&s.d, err) == 0);
  PrTaps t;
  REQUIRE(pr_build_taps(&s.d, t, err) == 0);
  REQUIRE(t.maxtaps >= 1 && t.maxtaps <= PR_MAXTAPS);
  // the tap list against the dense product, for one command vector
  const int npts = s.d.npts;
  std::vector<double> com(s.nact), want(npts, 0.0);
  for (int a = 0; a < s.nact; a++) com[a] = sin(1.0 + a);
  for (int a = 0; a < s.nact; a++)
    for (int j = s.indptr[a]; j < s.indptr[a + 1]; j++) want[s.indices[j]] += (double)s.data[j] * com[a];
  for (int i = 0; i < npts; i++) {
    double got = 0.0;
    for (int k = 0; k < PR_MAXTAPS; k++) got += (double)t.w[(size_t)k * npts + i] * com[t.idx[(size_t)k * npts + i]];
    REQUIRE(fabs(got - want[i]) <= 1e-12);
  }
  // more than 16 influence functions over a pixel
  make(s, 33, 128, 6, 40.0);
  REQUIRE(pr_validate(&s.d, err) == 0 && pr_build_taps(&s.d, t, err) == 1 && err.find("more than 16") != std::string::npos);
  // every refusal of the validator, by the field it names
  make(s, 24, 64, 4, 8.0);
  REQUIRE(pr_validate(nullptr, err) == 1);
  const int sizes[] = {4096, 16, 96, 0, -64};
  for (int n : sizes) {
    aomarl_psfrec_desc d = s.d;
    d.N = n;
    REQUIRE(pr_validate(&d, err) == 1 && err.find("N = ") != std::string::npos);
  }
  { aomarl_psfrec_desc d = s.d; d.p = 40; REQUIRE(pr_validate(&d, err) == 1 && err.find("p = 40") != std::string::npos); }
  { aomarl_psfrec_desc d = s.d; d.npts = 24 * 24 + 1; REQUIRE(pr_validate(&d, err) == 1 && err.find("npts") != std::string::npos); }
  { aomarl_psfrec_desc d = s.d; d.nactu = 2; REQUIRE(pr_validate(&d, err) == 1 && err.find("nactu") != std::string::npos); }
  { aomarl_psfrec_desc d = s.d; d.ld_actu = d.nactu - 1; REQUIRE(pr_validate(&d, err) == 1 && err.find("ld_actu") != std::string::npos); }
  { aomarl_psfrec_desc d = s.d; d.tt = nullptr; REQUIRE(pr_validate(&d, err) == 1 && err.find("null array") != std::string::npos); }
  { aomarl_psfrec_desc d = s.d; d.if_data = nullptr; REQUIRE(pr_validate(&d, err) == 1 && err.find("if_data") != std::string::npos); }
  { std::vector<int32_t> ip(s.indptr.size(), 0); aomarl_psfrec_desc d = s.d; d.if_indptr = ip.data(); d.if_data = nullptr;
    d.if_indices = nullptr;                                  // no influence function at all: tip and tilt only
    REQUIRE(pr_validate(&d, err) == 0 && pr_build_taps(&d, t, err) == 0 && t.maxtaps == 0); }
  { std::vector<int32_t> l = s.lit; l[3] = l[2]; aomarl_psfrec_desc d = s.d; d.lit = l.data();
    REQUIRE(pr_validate(&d, err) == 1 && err.find("lit[3]") != std::string::npos); }
  { std::vector<int32_t> l = s.lit; l.back() = 24 * 24; aomarl_psfrec_desc d = s.d; d.lit = l.data();
    REQUIRE(pr_validate(&d, err) == 1 && err.find("lit[") != std::string::npos); }
  { std::vector<int32_t> ip = s.indptr; ip[0] = 1; aomarl_psfrec_desc d = s.d; d.if_indptr = ip.data();
    REQUIRE(pr_validate(&d, err) == 1 && err.find("if_indptr[0]") != std::string::npos); }
  { std::vector<int32_t> ip = s.indptr; ip[2] = ip[1] - 1; aomarl_psfrec_desc d = s.d; d.if_indptr = ip.data();
    REQUIRE(pr_validate(&d, err) == 1 && err.find("decreases") != std::string::npos); }
  { std::vector<int32_t> ix = s.indices; ix[5] = s.d.npts; aomarl_psfrec_desc d = s.d; d.if_indices = ix.data();
    REQUIRE(pr_validate(&d, err) == 1 && err.find("if_indices[5]") != std::string::npos); }
  { std::vector<int32_t> ix = s.indices; ix[0] = -1; aomarl_psfrec_desc d = s.d; d.if_indices = ix.data();
    REQUIRE(pr_validate(&d, err) == 1 && err.find("if_indices[0]") != std::string::npos); }
  printf("psfrec_host_check: ok\n");
  return 0;
}
