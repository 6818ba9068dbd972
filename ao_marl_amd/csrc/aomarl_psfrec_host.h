// aomarl_psfrec_host.h -- the host half of aomarl_psfrec_create (aomarl_psfrec.hip): validation of the desc and the
// per-pixel tap list of the influence functions.  Plain C++ without a HIP call, so that it also compiles into a
// stand-alone host program (psfrec_host_check.cpp) that runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/aomarl.h"

#define PR_MAXTAPS 16
#define PR_NMIN 32
#define PR_NMAX 2048

struct PrTaps {
  std::vector<int32_t> idx;   // [PR_MAXTAPS][npts], actuator of tap t of pixel i at idx[t * npts + i]; unused taps: 0
  std::vector<float> w;       // the same layout; unused taps: 0.f
  int maxtaps = 0;            // most taps on one pixel
};

static inline std::string pr_fmt(const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  return std::string(buf);
}

// 0 when the desc can be used; otherwise 1 and `err` names the field
static inline int pr_validate(const aomarl_psfrec_desc *d, std::string &err) {
  if (!d) { err = "psfrec_create: null desc"; return 1; }
  if (d->N < PR_NMIN || d->N > PR_NMAX || (d->N & (d->N - 1)))
    { err = pr_fmt("psfrec_create: N = %lld: the transform size must be a power of two in 32..2048", d->N); return 1; }
  if (d->p < 1 || 2LL * d->p > d->N)
    { err = pr_fmt("psfrec_create: p = %lld with N = %lld: the pupil must fit half the grid (N >= 2 p)", d->p, d->N); return 1; }
  if (d->npts < 1 || (long long)d->npts > (long long)d->p * d->p)
    { err = pr_fmt("psfrec_create: npts = %lld lit pixels on a %lld x %lld pupil", d->npts, d->p, d->p); return 1; }
  if (d->nactu < 3 || d->ld_actu < d->nactu)
    { err = pr_fmt("psfrec_create: nactu = %lld (stack array + tip + tilt), ld_actu = %lld", d->nactu, d->ld_actu); return 1; }
  if (!d->lit || !d->if_indptr || !d->tt || !d->denmask || !d->mask || !d->otftel)
    { err = "psfrec_create: null array in the desc"; return 1; }
  long long prev = -1;
  for (int i = 0; i < d->npts; i++) {
    const long long v = d->lit[i];
    if (v <= prev || v >= (long long)d->p * d->p)
      { err = pr_fmt("psfrec_create: lit[%lld] = %lld: indices must ascend within the %lld pixels of the pupil", i, v,
                     (long long)d->p * d->p); return 1; }
    prev = v;
  }
  const int nrow = d->nactu - 2;
  if (d->if_indptr[0] != 0) { err = "psfrec_create: if_indptr[0] must be 0"; return 1; }
  for (int a = 0; a < nrow; a++)
    if (d->if_indptr[a + 1] < d->if_indptr[a])
      { err = pr_fmt("psfrec_create: if_indptr decreases at row %lld", a); return 1; }
  const long long nnz = d->if_indptr[nrow];
  if (nnz > 0 && (!d->if_data || !d->if_indices))          // a matrix without entries may come without arrays
    { err = "psfrec_create: null if_data / if_indices in the desc"; return 1; }
  for (long long j = 0; j < nnz; j++)
    if (d->if_indices[j] < 0 || d->if_indices[j] >= d->npts)
      { err = pr_fmt("psfrec_create: if_indices[%lld] = %lld outside the %lld lit pixels", j, d->if_indices[j], d->npts);
        return 1; }
  return 0;
}

// CSR [nactu - 2][npts] (one row per actuator) -> taps per pixel, in actuator order.  Call after pr_validate.
static inline int pr_build_taps(const aomarl_psfrec_desc *d, PrTaps &t, std::string &err) {
  const size_t npts = (size_t)d->npts;
  t.idx.assign(PR_MAXTAPS * npts, 0);
  t.w.assign(PR_MAXTAPS * npts, 0.f);
  std::vector<int> count(npts, 0);
  t.maxtaps = 0;
  for (int a = 0; a < d->nactu - 2; a++)
    for (int32_t j = d->if_indptr[a]; j < d->if_indptr[a + 1]; j++) {
      const float v = d->if_data[j];
      if (v == 0.f) continue;
      const size_t px = (size_t)d->if_indices[j];
      const int n = count[px];
      if (n >= PR_MAXTAPS)
        { err = pr_fmt("psfrec_create: lit pixel %lld is under more than %lld influence functions", (long long)px,
                       PR_MAXTAPS); return 1; }
      t.idx[(size_t)n * npts + px] = a;
      t.w[(size_t)n * npts + px] = v;
      count[px] = n + 1;
      if (n + 1 > t.maxtaps) t.maxtaps = n + 1;
    }
  return 0;
}
