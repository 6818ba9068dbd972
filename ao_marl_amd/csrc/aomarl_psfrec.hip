// aomarl_psfrec.hip -- PSF reconstruction from the covariance of the ROKET error buffers, the Vii algorithm
// (reference: guardians/gamora.py:103-171 psf_rec_vii_cpu, :24-100 psf_rec_Vii).  gfx950 only.
//
// Per eigenmode of the covariance the reference transforms two zero-padded N x N maps.  The first of them enters
// linearly, so  sum_k e_k fft2(m_k^2) = fft2(sum_k e_k m_k^2): one variance map per environment.  What is left per mode
// is  acc += e_k |fft2 m_k|^2  of a real map that is zero outside p rows and p columns:
//   k_pr_synth   m_k on the lit pixels from the per-pixel tap list (<= 16 taps + tip + tilt), var += w_k m_k^2.
//                One thread owns one lit pixel and walks the modes of the batch in order.
//   k_pr_rows    two real rows packed into one complex line (z = row_a + i row_b), one N-point transform in LDS,
//                split into the two half spectra, N/2 + 1 columns kept -> T [mode][row][column]
//   k_pr_cols    CW adjacent columns of T per workgroup (CW * 8 bytes per row: whole 64-byte pieces for CW = 8), p
//                non-zero rows, N-point transforms in LDS, acc += w_k |.|^2 in registers over the modes of the batch.
//                One thread owns its elements of acc and adds the modes in order: no atomics, same bits however the
//                modes are split into calls and batches.
// The transform (pr_fft_lds, aomarl_fft_lds.h) is an in-place radix-2 decimation-in-frequency pass over lines held in LDS: natural order
// in, bit-reversed order out, twiddles from a table.  Nothing is ever un-scrambled on the hot path: the row pass keeps
// its columns, and the column pass its rows, in LDS position order (T's column c holds frequency brev(2c), column N/2
// frequency N/2; acc's row q holds frequency brev(q)); the split of the packed rows pairs position q with
// q ^ (2^floor(log2 q) - 1), which is where frequency N - k lies.  k_pr_tmp undoes both once per environment.
// LDS layout: element i of line c lies at slot sw(i) * CW + c, sw(i) = i ^ (G - 1 where bit G of i is set), G = 32 / CW.
// A half wave (the conflict group of the 8-byte LDS accesses) handles G butterflies of CW lines; at stride s < G its
// elements are those of an aligned span of 2 G with bit s clear (or set), and the swizzle sends the two halves of that
// span to complementary slots: every stage reads and writes 32 distinct 8-byte slots of the 256-byte bank row.
// The finish (once per environment) runs whole complex transforms through k_pr_fft_t, one line per workgroup with a
// transposed, un-scrambled store; two of them make a 2-D transform.
#include "aomarl_host.h"
#include "aomarl_psfrec_host.h"
#include "aomarl_fft_lds.h"
#include <math.h>
#include <string.h>

#define PR_THREADS 256
#define PR_MAX_BATCH 32
// bytes of T and maps a batch of modes may occupy: well inside the 256 MB last-level cache, so that the row pass's
// output is still there when the column pass reads it
#define PR_BATCH_BYTES (96ll << 20)

// --------------------------------------------------------------------------------------------------- per mode
// maps [nb][p][p] (only lit pixels are ever written, the rest stays zero), var [npts]
__global__ void k_pr_synth(const float *__restrict__ com, int ld, const float *__restrict__ w, int nb, int nactu,
                           const int *__restrict__ lit, const int *__restrict__ tap_i, const float *__restrict__ tap_w,
                           int maxtaps, const float *__restrict__ tt, int npts, int pp, float *__restrict__ maps,
                           float *__restrict__ var) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npts) return;
  int ti[PR_MAXTAPS];
  float tw[PR_MAXTAPS];
#pragma unroll
  for (int t = 0; t < PR_MAXTAPS; t++) {
    const bool on = t < maxtaps;
    ti[t] = on ? tap_i[(size_t)t * npts + i] : 0;
    tw[t] = on ? tap_w[(size_t)t * npts + i] : 0.f;
  }
  const float t0 = tt[2 * i], t1 = tt[2 * i + 1];
  const int px = lit[i];
  float v = var[i];
  for (int b = 0; b < nb; b++) {
    const float *c = com + (size_t)b * ld;
    float m = 0.f;
#pragma unroll
    for (int t = 0; t < PR_MAXTAPS; t++) m += tw[t] * c[ti[t]];
    m += t0 * c[nactu - 2] + t1 * c[nactu - 1];
    maps[(size_t)b * pp + px] = m;
    v += w[b] * (m * m);
  }
  var[i] = v;
}

// grid (row pairs, modes).  T [mode][2 npairs][ldt]
__global__ __launch_bounds__(PR_THREADS) void k_pr_rows(const float *__restrict__ maps, int p, int logn,
                                                         float2 *__restrict__ T, long long t_stride, int ldt,
                                                         const float2 *__restrict__ tw) {
  __shared__ float2 x[PR_NMAX];
  const int N = 1 << logn, tid = threadIdx.x, nt = blockDim.x;
  const int r = blockIdx.x, b = blockIdx.y;
  const float *m0 = maps + (size_t)b * p * p + (size_t)(2 * r) * p;
  const bool has1 = 2 * r + 1 < p;
  for (int i = tid; i < N; i += nt) {
    float2 v = make_float2(0.f, 0.f);
    if (i < p) {
      v.x = m0[i];
      if (has1) v.y = m0[p + i];
    }
    x[pr_sw<1>(i)] = v;
  }
  __syncthreads();
  pr_fft_lds<1>(x, logn, tw, false, tid, nt);
  float2 *Ta = T + (size_t)b * t_stride + (size_t)(2 * r) * ldt, *Tb = Ta + ldt;
  for (int c = tid; c <= N / 2; c += nt) {
    const int q = c == N / 2 ? 1 : 2 * c;
    const int qp = q ? q ^ ((1 << (31 - __clz(q))) - 1) : 0;       // where frequency N - k lies
    const float2 zq = x[pr_sw<1>(q)], zp = x[pr_sw<1>(qp)];
    Ta[c] = make_float2(0.5f * (zq.x + zp.x), 0.5f * (zq.y - zp.y));
    Tb[c] = make_float2(0.5f * (zq.y + zp.y), -0.5f * (zq.x - zp.x));
  }
}

// grid: groups of CW columns.  acc [N][ldacc], row = LDS position of the column transform
template <int LOGN, int CW>
__global__ __launch_bounds__(PR_THREADS) void k_pr_cols(const float2 *__restrict__ T, long long t_stride, int ldt, int p,
                                                         int ncols, const float *__restrict__ w, int nb,
                                                         float *__restrict__ acc, int ldacc, const float2 *__restrict__ tw) {
  constexpr int N = 1 << LOGN, SLOTS = N * CW, R = (SLOTS + PR_THREADS - 1) / PR_THREADS;
  __shared__ float2 x[SLOTS];
  const int tid = threadIdx.x, col0 = blockIdx.x * CW;
  float a[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int slot = tid + r * PR_THREADS, pos = slot / CW, col = col0 + slot % CW;
    a[r] = (slot < SLOTS && col < ncols) ? acc[(size_t)pr_sw<CW>(pos) * ldacc + col] : 0.f;
  }
  for (int b = 0; b < nb; b++) {
    const float2 *Tb = T + (size_t)b * t_stride;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int slot = tid + r * PR_THREADS, pos = slot / CW, col = col0 + slot % CW;
      if (slot < SLOTS) {
        const int y = pr_sw<CW>(pos);
        x[slot] = (y < p && col < ncols) ? Tb[(size_t)y * ldt + col] : make_float2(0.f, 0.f);
      }
    }
    __syncthreads();
    pr_fft_lds<CW>(x, LOGN, tw, false, tid, PR_THREADS);
    const float wb = w[b];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int slot = tid + r * PR_THREADS;
      if (slot < SLOTS) {
        const float2 z = x[slot];
        a[r] += wb * (z.x * z.x + z.y * z.y);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int slot = tid + r * PR_THREADS, pos = slot / CW, col = col0 + slot % CW;
    if (slot < SLOTS && col < ncols) acc[(size_t)pr_sw<CW>(pos) * ldacc + col] = a[r];
  }
}

// --------------------------------------------------------------------------------------------------- finish
// one line per workgroup: out[k][line] = sum_i in[line][i] exp(-+ 2 pi i k i / N)
__global__ __launch_bounds__(PR_THREADS) void k_pr_fft_t(const float2 *__restrict__ in, float2 *__restrict__ out, int logn,
                                                          int inv, const float2 *__restrict__ tw) {
  __shared__ float2 x[PR_NMAX];
  const int N = 1 << logn, tid = threadIdx.x, nt = blockDim.x, line = blockIdx.x;
  for (int i = tid; i < N; i += nt) x[pr_sw<1>(i)] = in[(size_t)line * N + i];
  __syncthreads();
  pr_fft_lds<1>(x, logn, tw, inv != 0, tid, nt);
  for (int q = tid; q < N; q += nt) out[(size_t)pr_brev(q, logn) * N + line] = x[pr_sw<1>(q)];
}

// dst [N][N] complex, zeroed by the caller: the lit pixels of the p x p corner take src (or 1 where src is NULL)
__global__ void k_pr_scatter(const float *__restrict__ src, const int *__restrict__ lit, int npts, int p, int N,
                             float2 *__restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npts) return;
  const int px = lit[i], y = px / p;
  dst[(size_t)y * N + (px - y * p)] = make_float2(src ? src[i] : 1.f, 0.f);
}

// B = 2 (Re(A conj(Pf)) - acc), acc read through its two permutations and, for kx > N/2, through the symmetry of the
// spectrum of a real map
__global__ void k_pr_tmp(const float2 *__restrict__ A, const float2 *__restrict__ Pf, const float *__restrict__ acc,
                         int ldacc, int logn, float2 *__restrict__ B) {
  const int N = 1 << logn;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * N) return;
  const int ky = (int)(i >> logn), kx = (int)(i & (N - 1));
  const bool lo = kx <= N / 2;
  const int kxx = lo ? kx : N - kx, kyy = lo ? ky : (N - ky) & (N - 1);
  const int c = kxx == N / 2 ? N / 2 : pr_brev(kxx, logn) >> 1;
  const float av = acc[(size_t)pr_brev(kyy, logn) * ldacc + c];
  const float2 a = A[i], f = Pf[i];
  B[i] = make_float2(2.f * ((a.x * f.x + a.y * f.y) - av), 0.f);
}

// dphi = Re(B) / N^2 . denmask; E = exp(-dphi / 2) . mask; part[block] = max of the block's E
__global__ __launch_bounds__(PR_THREADS) void k_pr_tail1(const float2 *__restrict__ B, const float *__restrict__ denmask,
                                                          const float *__restrict__ mask, long long n, float inv_n2,
                                                          float *__restrict__ dphi, float *__restrict__ E,
                                                          float *__restrict__ part) {
  __shared__ float red[PR_THREADS];
  float mx = 0.f;                                             // E >= 0
  for (long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * PR_THREADS) {
    const float d = B[i].x * inv_n2 * denmask[i];
    const float e = expf(-0.5f * d) * mask[i];
    if (dphi) dphi[i] = d;
    E[i] = e;
    mx = fmaxf(mx, e);
  }
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int s = PR_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// otf2 = E / max(part); A = otf_other . otf2
__global__ __launch_bounds__(PR_THREADS) void k_pr_tail2(const float *__restrict__ E, const float *__restrict__ part,
                                                          int nparts, const float *__restrict__ other, long long n,
                                                          float *__restrict__ otf2, float2 *__restrict__ A) {
  float mx = 0.f;
  for (int j = 0; j < nparts; j++) mx = fmaxf(mx, part[j]);   // every thread, the same order
  const long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= n) return;
  const float o = E[i] / mx;
  if (otf2) otf2[i] = o;
  A[i] = make_float2(other[i] * o, 0.f);
}

// psf = fftshift(Re A) . scale
__global__ void k_pr_psf(const float2 *__restrict__ A, int logn, float scale, float *__restrict__ psf) {
  const int N = 1 << logn;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * N) return;
  const int y = (int)(i >> logn), x = (int)(i & (N - 1));
  psf[(size_t)((y + N / 2) & (N - 1)) * N + ((x + N / 2) & (N - 1))] = A[i].x * scale;
}

// ------------------------------------------------------------------------------------------------- host side
#define PR_PARTS 256
struct aomarl_psfrec {
  int p, N, logn, npts, nactu, ld_in, maxtaps, batch, npairs, ncols, ldt, ldacc, cw;
  long long t_stride;
  int *lit, *tap_i;
  float *tap_w, *tt, *denmask, *mask, *otftel, *var, *acc, *maps, *E, *part;
  float2 *tw, *T, *Pf, *A, *B;
};

static inline unsigned pr_blocks(long long total) { return (unsigned)((total + PR_THREADS - 1) / PR_THREADS); }
static inline int pr_line_threads(int N) { return N / 2 < 64 ? 64 : (N / 2 > PR_THREADS ? PR_THREADS : N / 2); }

int aomarl_psfrec_destroy(aomarl_psfrec *r) {
  if (!r) return 0;
  void *q[] = {r->lit, r->tap_i, r->tap_w, r->tt, r->denmask, r->mask, r->otftel, r->var, r->acc, r->maps, r->E, r->part,
               r->tw, r->T, r->Pf, r->A, r->B};
  for (void *v : q) if (v) (void)hipFree(v);
  delete r;
  return 0;
}

int aomarl_psfrec_reset(aomarl_psfrec *r) {
  if (!r) return fail("psfrec_reset: null object");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(r->var, 0, (size_t)r->npts * sizeof(float)));
  HIPCHK(hipMemset(r->acc, 0, (size_t)r->N * r->ldacc * sizeof(float)));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

// dst = fft2(src) (inv: the un-normalised inverse), both [N][N]; tmp is overwritten.  dst may be src.
static int pr_fft2(aomarl_psfrec *r, const float2 *src, float2 *tmp, float2 *dst, int inv, hipStream_t s) {
  const int nt = pr_line_threads(r->N);
  k_pr_fft_t<<<r->N, nt, 0, s>>>(src, tmp, r->logn, inv, r->tw);
  LAUNCHCHK();
  k_pr_fft_t<<<r->N, nt, 0, s>>>(tmp, dst, r->logn, inv, r->tw);
  LAUNCHCHK();
  return 0;
}

int aomarl_psfrec_create(const aomarl_psfrec_desc *d, aomarl_psfrec **out) {
  if (!out) return fail("psfrec_create: null argument");
  std::string err;
  PrTaps taps;
  if (pr_validate(d, err) || pr_build_taps(d, taps, err)) return fail("%s", err.c_str());
  aomarl_psfrec *r = new aomarl_psfrec();
  memset(r, 0, sizeof(*r));
  r->p = d->p; r->N = d->N; r->npts = d->npts; r->nactu = d->nactu; r->ld_in = d->ld_actu;
  r->maxtaps = taps.maxtaps;
  for (r->logn = 0; (1 << r->logn) < r->N; r->logn++) {}
  r->npairs = (r->p + 1) / 2;
  r->ncols = r->N / 2 + 1;
  r->ldt = r->N / 2 + 8;            // rows of T and acc begin on 64 / 32-byte boundaries
  r->ldacc = r->N / 2 + 8;
  r->cw = r->N <= 1024 ? 8 : 4;     // CW lines of N complex numbers: at most 64 KB of LDS
  r->t_stride = (long long)2 * r->npairs * r->ldt;
  const long long per_mode = r->t_stride * (long long)sizeof(float2) + (long long)r->p * r->p * (long long)sizeof(float);
  long long nb = PR_BATCH_BYTES / per_mode;
  r->batch = (int)(nb < 1 ? 1 : (nb > PR_MAX_BATCH ? PR_MAX_BATCH : nb));
  const size_t n2 = (size_t)r->N * r->N, npts = (size_t)r->npts;
  std::vector<float2> htw((size_t)r->N / 2);
  for (int j = 0; j < r->N / 2; j++) {
    const double a = -2.0 * M_PI * (double)j / (double)r->N;
    htw[j] = make_float2((float)cos(a), (float)sin(a));
  }
  bool ok = hipMalloc((void **)&r->lit, npts * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&r->tap_i, PR_MAXTAPS * npts * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&r->tap_w, PR_MAXTAPS * npts * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->tt, 2 * npts * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->denmask, n2 * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->mask, n2 * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->otftel, n2 * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->var, npts * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->acc, (size_t)r->N * r->ldacc * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->maps, (size_t)r->batch * r->p * r->p * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->E, n2 * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->part, PR_PARTS * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&r->tw, htw.size() * sizeof(float2)) == hipSuccess &&
            hipMalloc((void **)&r->T, (size_t)r->batch * r->t_stride * sizeof(float2)) == hipSuccess &&
            hipMalloc((void **)&r->Pf, n2 * sizeof(float2)) == hipSuccess &&
            hipMalloc((void **)&r->A, n2 * sizeof(float2)) == hipSuccess &&
            hipMalloc((void **)&r->B, n2 * sizeof(float2)) == hipSuccess;
  ok = ok && hipMemcpy(r->lit, d->lit, npts * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->tap_i, taps.idx.data(), PR_MAXTAPS * npts * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->tap_w, taps.w.data(), PR_MAXTAPS * npts * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->tt, d->tt, 2 * npts * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->denmask, d->denmask, n2 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->mask, d->mask, n2 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->otftel, d->otftel, n2 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(r->tw, htw.data(), htw.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(r->maps, 0, (size_t)r->batch * r->p * r->p * sizeof(float)) == hipSuccess &&
       hipMemset(r->T, 0, (size_t)r->batch * r->t_stride * sizeof(float2)) == hipSuccess &&
       hipMemset(r->A, 0, n2 * sizeof(float2)) == hipSuccess;
  if (ok) {                                                   // Pf = fft2(pup)
    k_pr_scatter<<<pr_blocks(r->npts), PR_THREADS, 0, 0>>>(nullptr, r->lit, r->npts, r->p, r->N, r->A);
    ok = hipGetLastError() == hipSuccess && pr_fft2(r, r->A, r->B, r->Pf, 0, 0) == 0;
  }
  if (!ok || aomarl_psfrec_reset(r)) {
    aomarl_psfrec_destroy(r);
    return fail("psfrec_create: device allocation or the pupil transform failed (p %d, N %d, %d lit pixels)", d->p, d->N,
                d->npts);
  }
  *out = r;
  return 0;
}

template <int LOGN, int CW>
static void pr_launch_cols(aomarl_psfrec *r, const float *w, int nb, hipStream_t s) {
  k_pr_cols<LOGN, CW><<<(r->ncols + CW - 1) / CW, PR_THREADS, 0, s>>>(r->T, r->t_stride, r->ldt, r->p, r->ncols, w, nb, r->acc,
                                                                     r->ldacc, r->tw);
}

int aomarl_psfrec_accumulate(aomarl_psfrec *r, const float *com, const float *w, int nk, void *stream) {
  if (!r) return fail("psfrec_accumulate: null object");
  if (!com || !w) return fail("psfrec_accumulate: null input");
  if (nk < 1) return fail("psfrec_accumulate: nk = %d", nk);
  hipStream_t s = (hipStream_t)stream;
  for (int k0 = 0; k0 < nk; k0 += r->batch) {
    const int nb = nk - k0 < r->batch ? nk - k0 : r->batch;
    const float *cb = com + (size_t)k0 * r->ld_in, *wb = w + k0;
    k_pr_synth<<<pr_blocks(r->npts), PR_THREADS, 0, s>>>(cb, r->ld_in, wb, nb, r->nactu, r->lit, r->tap_i, r->tap_w, r->maxtaps,
                                                         r->tt, r->npts, r->p * r->p, r->maps, r->var);
    LAUNCHCHK();
    k_pr_rows<<<dim3(r->npairs, nb), pr_line_threads(r->N), 0, s>>>(r->maps, r->p, r->logn, r->T, r->t_stride, r->ldt, r->tw);
    LAUNCHCHK();
    switch (r->logn) {
      case 5: pr_launch_cols<5, 8>(r, wb, nb, s); break;
      case 6: pr_launch_cols<6, 8>(r, wb, nb, s); break;
      case 7: pr_launch_cols<7, 8>(r, wb, nb, s); break;
      case 8: pr_launch_cols<8, 8>(r, wb, nb, s); break;
      case 9: pr_launch_cols<9, 8>(r, wb, nb, s); break;
      case 10: pr_launch_cols<10, 8>(r, wb, nb, s); break;
      case 11: pr_launch_cols<11, 4>(r, wb, nb, s); break;
      default: return fail("psfrec_accumulate: N = %d", r->N);
    }
    LAUNCHCHK();
  }
  return 0;
}

int aomarl_psfrec_finish(aomarl_psfrec *r, const float *otf_other, float *dphi, float *otf2, float *psf, void *stream) {
  if (!r) return fail("psfrec_finish: null object");
  hipStream_t s = (hipStream_t)stream;
  const long long n2 = (long long)r->N * r->N;
  HIPCHK(hipMemsetAsync(r->A, 0, n2 * sizeof(float2), s));
  k_pr_scatter<<<pr_blocks(r->npts), PR_THREADS, 0, s>>>(r->var, r->lit, r->npts, r->p, r->N, r->A);
  LAUNCHCHK();
  if (pr_fft2(r, r->A, r->B, r->A, 0, s)) return 1;
  k_pr_tmp<<<pr_blocks(n2), PR_THREADS, 0, s>>>(r->A, r->Pf, r->acc, r->ldacc, r->logn, r->B);
  LAUNCHCHK();
  if (pr_fft2(r, r->B, r->A, r->B, 1, s)) return 1;
  const long long want = (n2 + PR_THREADS - 1) / PR_THREADS;
  const int nparts = (int)(want < PR_PARTS ? want : PR_PARTS);
  k_pr_tail1<<<nparts, PR_THREADS, 0, s>>>(r->B, r->denmask, r->mask, n2, 1.f / (float)n2, dphi, r->E, r->part);
  LAUNCHCHK();
  k_pr_tail2<<<pr_blocks(n2), PR_THREADS, 0, s>>>(r->E, r->part, nparts, otf_other ? otf_other : r->otftel, n2, otf2, r->A);
  LAUNCHCHK();
  if (psf) {
    if (pr_fft2(r, r->A, r->B, r->A, 1, s)) return 1;
    k_pr_psf<<<pr_blocks(n2), PR_THREADS, 0, s>>>(r->A, r->logn, 1.f / (float)r->npts, psf);   // 1/N^2 . N^2/npts
    LAUNCHCHK();
  }
  return 0;
}
