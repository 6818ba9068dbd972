// aomarl_pyr.hip -- the pyramid wavefront sensor ("pyrhr": four pupil images, modulation, field stop).  gfx950 only.
// The model is ao_marl_amd/pyramid.py:PyramidModel (float64 NumPy); the geometry is geometry.pyr_geometry (reference:
// shesha/init/geom_init.py:init_pyrhr_geom, the image formation itself is not in the reference tree).
//
// Per (environment, modulation point) two Nfft^2 complex transforms whose input has n lit rows, in three passes over
// lines held in LDS (aomarl_fft_lds.h):
//   k_pyr_rows   one lit row per workgroup: the field mpupil exp(i (2 pi / lambda phi + cx (x - n/2) + cy (y - n/2))) is
//                formed on the fly, transformed forward (decimation in frequency: the columns of T1 [pair][n][Nfft] stay
//                in LDS position order, column q holds frequency brev(q))
//   k_pyr_cols   CW adjacent columns per workgroup, one LDS residency: forward, x the pyramid phasor and field stop,
//                inverse (decimation in time, which takes the scrambled order in and gives the natural order out).  The
//                mask is permuted at create time (maskp[i][q] = mask[brev(i)][brev(q)] / Nfft): nothing is unscrambled.
//                -> T2 [pair][Nfft][Nfft], rows in natural order
//   k_pyr_irows  one row of one environment per workgroup, over the modulation points of the batch in index order:
//                inverse transform of the row, hr += w_k |.|^2 in registers.  One thread owns its pixels of hr: no
//                atomics, the same bits however the environments are split into calls and the points into batches.
// Then the pixel filter (k_pyr_fft_t, four whole-line passes per frame), k_pyr_bin (sums over nrebin^2 blocks, flux
// scale, noise) and k_pyr_slopes (one workgroup per environment: the mean intensity in a fixed order, the slopes).
#include "aomarl_host.h"
#include "aomarl_pyr_host.h"
#include "aomarl_fft_lds.h"
#include <math.h>
#include <string.h>
#include <vector>

#define PYR_THREADS 256

// a pair of the batch: environment env0 + b / pts_b, point k0 + b % pts_b
// grid (n lit rows, pairs).  T1 [pair][n][N]
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_rows(const float *__restrict__ phase, const float *__restrict__ mpupil,
                                                           const float *__restrict__ cx, const float *__restrict__ cy, int n,
                                                           int logn, int env0, int k0, int pts_b, float k2pi,
                                                           float2 *__restrict__ T1, const float2 *__restrict__ tw) {
  __shared__ float2 x[PYR_NMAX];
  const int N = 1 << logn, tid = threadIdx.x, nt = blockDim.x;
  const int r = blockIdx.x, b = blockIdx.y, e = env0 + b / pts_b, k = k0 + b % pts_b;
  const int off = N / 2 - n / 2;
  const float ax = cx[k], ay = cy[k] * (float)(r - n / 2);
  const float *ph = phase + (size_t)e * n * n + (size_t)r * n, *mp = mpupil + (size_t)r * n;
  for (int i = tid; i < N; i += nt) {
    float2 v = make_float2(0.f, 0.f);
    const int c = i - off;
    if (c >= 0 && c < n) {
      const float m = mp[c];
      if (m != 0.f) {
        float sn, cs;
        sincosf(k2pi * ph[c] + (ax * (float)(c - n / 2) + ay), &sn, &cs);
        v = make_float2(m * cs, m * sn);
      }
    }
    x[pr_sw<1>(i)] = v;
  }
  __syncthreads();
  pr_fft_lds<1>(x, logn, tw, false, tid, nt);
  float2 *out = T1 + ((size_t)b * n + r) * N;
  for (int q = tid; q < N; q += nt) out[q] = x[pr_sw<1>(q)];
}

// grid (N / CW column groups, pairs).  T2 [pair][N][N]
template <int LOGN, int CW>
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_cols(const float2 *__restrict__ T1, int n, const float2 *__restrict__ maskp,
                                                           float2 *__restrict__ T2, const float2 *__restrict__ tw) {
  constexpr int N = 1 << LOGN, SLOTS = N * CW, R = SLOTS / PYR_THREADS;
  static_assert(SLOTS % PYR_THREADS == 0, "whole rounds of the workgroup");
  __shared__ float2 x[SLOTS];
  const int tid = threadIdx.x, col0 = blockIdx.x * CW, b = blockIdx.y;
  const int off = N / 2 - n / 2;
  const float2 *in = T1 + (size_t)b * n * N;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int slot = tid + r * PYR_THREADS, i = pr_sw<CW>(slot / CW), col = col0 + slot % CW, y = i - off;
    x[slot] = (y >= 0 && y < n) ? in[(size_t)y * N + col] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  pr_fft_lds<CW>(x, LOGN, tw, false, tid, PYR_THREADS);
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int slot = tid + r * PYR_THREADS, i = pr_sw<CW>(slot / CW), col = col0 + slot % CW;
    const float2 z = x[slot], m = maskp[(size_t)i * N + col];
    x[slot] = make_float2(z.x * m.x - z.y * m.y, z.x * m.y + z.y * m.x);
  }
  __syncthreads();
  pr_fft_dit_lds<CW>(x, LOGN, tw, true, tid, PYR_THREADS);
  float2 *out = T2 + (size_t)b * N * N;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int slot = tid + r * PYR_THREADS, i = pr_sw<CW>(slot / CW), col = col0 + slot % CW;
    out[(size_t)i * N + col] = x[slot];
  }
}

// grid (N rows, environments of the batch).  hr [nenv][N][N]; first: this batch holds the first points of the frame
#define PYR_IROW_R (PYR_NMAX / PYR_THREADS)
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_irows(const float2 *__restrict__ T2, int logn, int env0, int k0, int pts_b,
                                                            const float *__restrict__ w, float wscale, int first,
                                                            float *__restrict__ hr, const float2 *__restrict__ tw) {
  __shared__ float2 x[PYR_NMAX];
  const int N = 1 << logn, tid = threadIdx.x, nt = blockDim.x;
  const int y = blockIdx.x, eb = blockIdx.y;
  float *h = hr + ((size_t)(env0 + eb) * N + y) * N;
  float a[PYR_IROW_R];
#pragma unroll
  for (int j = 0; j < PYR_IROW_R; j++) {
    const int i = tid + j * nt;
    a[j] = (!first && i < N) ? h[i] : 0.f;
  }
  for (int kk = 0; kk < pts_b; kk++) {
    const float2 *in = T2 + ((size_t)(eb * pts_b + kk) * N + y) * N;
    for (int q = tid; q < N; q += nt) x[pr_sw<1>(q)] = in[q];
    __syncthreads();
    pr_fft_dit_lds<1>(x, logn, tw, true, tid, nt);
    const float wk = w[k0 + kk] * wscale;
#pragma unroll
    for (int j = 0; j < PYR_IROW_R; j++) {
      const int i = tid + j * nt;
      if (i < N) {
        const float2 z = x[pr_sw<1>(i)];
        a[j] += wk * (z.x * z.x + z.y * z.y);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < PYR_IROW_R; j++) {
    const int i = tid + j * nt;
    if (i < N) h[i] = a[j];
  }
}

// ------------------------------------------------------------------------------------------------ pixel filter
// one line per workgroup, grid (N lines, planes): out[plane][k][line] = sum_i in[plane][line][i] exp(-+ 2 pi i k i / N),
// in: rin (real, planes rin_stride floats apart) or cin; x mul[k][line] when given; out: cout, or the real part x scale
// into rout
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_fft_t(const float *__restrict__ rin, const float2 *__restrict__ cin,
                                                            float2 *__restrict__ cout, float *__restrict__ rout,
                                                            const float *__restrict__ mul, float scale, int logn, int inv,
                                                            const float2 *__restrict__ tw) {
  __shared__ float2 x[PYR_NMAX];
  const int N = 1 << logn, tid = threadIdx.x, nt = blockDim.x, line = blockIdx.x;
  const size_t plane = (size_t)blockIdx.y * N * N;
  for (int i = tid; i < N; i += nt)
    x[pr_sw<1>(i)] = rin ? make_float2(rin[plane + (size_t)line * N + i], 0.f) : cin[plane + (size_t)line * N + i];
  __syncthreads();
  pr_fft_lds<1>(x, logn, tw, inv != 0, tid, nt);
  for (int q = tid; q < N; q += nt) {
    const size_t o = (size_t)pr_brev(q, logn) * N + line;
    float2 z = x[pr_sw<1>(q)];
    if (mul) { const float m = mul[o]; z.x *= m; z.y *= m; }
    if (rout) rout[plane + o] = z.x * scale;
    else cout[plane + o] = z;
  }
}

// ------------------------------------------------------------------------------------------------ image and slopes
// grid (blocks of pixels, environments).  img [nenv][nb * nb]
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_bin(const float *__restrict__ hr, int N, int nrebin, int env0, float scale,
                                                          float sigma, int noisy, const uint32_t *__restrict__ seeds,
                                                          const uint32_t *__restrict__ frame, float *__restrict__ img,
                                                          float *__restrict__ img_out) {
  const int nb = N / nrebin, idx = blockIdx.x * PYR_THREADS + threadIdx.x, e = env0 + blockIdx.y;
  if (idx >= nb * nb) return;
  const int by = idx / nb, bx = idx - by * nb;
  const float *h = hr + (size_t)e * N * N + (size_t)by * nrebin * N + (size_t)bx * nrebin;
  float s = 0.f;
  for (int yy = 0; yy < nrebin; yy++)
    for (int xx = 0; xx < nrebin; xx++) s += h[(size_t)yy * N + xx];
  s *= scale;
  if (noisy) s = sh_noise(s, sigma, seeds[e], frame[e], (uint32_t)idx);
  img[(size_t)e * nb * nb + idx] = s;
  if (img_out) img_out[(size_t)e * nb * nb + idx] = s;
}

// one workgroup per environment
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_slopes(const float *__restrict__ img, int nb, int nvalid, int env0,
                                                             const int *__restrict__ vx, const int *__restrict__ vy, int method,
                                                             float thresh, float s_scale, const float *__restrict__ ref,
                                                             float *__restrict__ slopes, float *__restrict__ slopes_out,
                                                             uint32_t *__restrict__ frame, int bump) {
  __shared__ float red[PYR_THREADS];
  const int tid = threadIdx.x, e = env0 + blockIdx.x;
  const float *im = img + (size_t)e * nb * nb;
  float s = 0.f;
  for (int i = tid; i < nvalid; i += PYR_THREADS) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) t += im[vx[j * nvalid + i] * nb + vy[j * nvalid + i]];
    s += t;
  }
  red[tid] = s;
  __syncthreads();
  for (int h = PYR_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const float mean = red[0] / (float)nvalid;
  for (int i = tid; i < nvalid; i += PYR_THREADS) {
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = im[vx[j * nvalid + i] * nb + vy[j * nvalid + i]];
    const float tot = ((q[0] + q[1]) + q[2]) + q[3];
    const float norm = method >= 2 ? tot : mean;
    float sx = 0.f, sy = 0.f;
    if (!(norm < thresh) && norm != 0.f) {
      sx = ((q[1] + q[3]) - (q[0] + q[2])) / norm;
      sy = ((q[1] + q[2]) - (q[0] + q[3])) / norm;
      if (method & 1) {
        sx = sinf(1.57079632679489661923f * sx);
        sy = sinf(1.57079632679489661923f * sy);
      }
      sx *= s_scale;
      sy *= s_scale;
    }
    sx -= ref[i];
    sy -= ref[nvalid + i];
    float *o = slopes + (size_t)e * 2 * nvalid;
    o[i] = sx;
    o[nvalid + i] = sy;
    if (slopes_out) {
      slopes_out[(size_t)e * 2 * nvalid + i] = sx;
      slopes_out[(size_t)e * 2 * nvalid + nvalid + i] = sy;
    }
  }
  if (bump && tid == 0) frame[e] += 1u;
}

// ------------------------------------------------------------------------------------------------- host side
struct aomarl_pyr {
  int nenv, n, N, logn, nrebin, nb, nvalid, npts_max, npts, pixel_filter;
  float k2pi, nphotons, noise, thresh, s_scale;
  double lit, wsum;
  PyrPlan plan;
  float *mpupil, *sincar, *cx, *cy, *w, *ref, *hr, *img, *slopes;
  int *vx, *vy;
  float2 *tw, *maskp, *T1, *T2, *FA, *FB;
};

static inline int pyr_line_threads(int N) { return N / 2 < 64 ? 64 : (N / 2 > PYR_THREADS ? PYR_THREADS : N / 2); }

int aomarl_pyr_destroy(aomarl_pyr *p) {
  if (!p) return 0;
  void *q[] = {p->mpupil, p->sincar, p->cx, p->cy, p->w, p->ref, p->hr, p->img, p->slopes, p->vx, p->vy, p->tw, p->maskp,
               p->T1, p->T2, p->FA, p->FB};
  for (void *v : q) if (v) (void)hipFree(v);
  delete p;
  return 0;
}

static unsigned pyr_brev_host(unsigned q, int logn) {
  unsigned r = 0;
  for (int b = 0; b < logn; b++) r |= ((q >> b) & 1u) << (logn - 1 - b);
  return r;
}

int aomarl_pyr_create(const aomarl_pyr_desc *d, aomarl_pyr **out) {
  if (!out) return fail("pyr_create: null argument");
  std::string err;
  if (pyr_validate(d, err)) return fail("%s", err.c_str());
  aomarl_pyr *p = new aomarl_pyr();
  memset((void *)p, 0, sizeof(*p));
  p->nenv = d->nenv; p->n = d->n; p->N = d->Nfft; p->nrebin = d->nrebin; p->nb = d->Nfft / d->nrebin;
  p->nvalid = d->nvalid; p->npts_max = d->npts_max; p->pixel_filter = d->pixel_filter != 0;
  for (p->logn = 0; (1 << p->logn) < p->N; p->logn++) {}
  p->k2pi = (float)(2.0 * M_PI / (double)d->lambda_um);
  p->nphotons = d->nphotons; p->noise = d->noise; p->thresh = d->thresh; p->s_scale = 1.f;
  p->npts = 1; p->wsum = 1.0;
  p->lit = 0;
  for (long long i = 0; i < (long long)d->n * d->n; i++) p->lit += (double)d->mpupil[i] * d->mpupil[i];
  p->plan = pyr_plan(p->n, p->N, p->nenv, p->npts_max, d->batch_kib ? (long long)d->batch_kib << 10 : PYR_BATCH_BYTES);
  const int N = p->N;
  const size_t n2 = (size_t)N * N, nn = (size_t)p->n * p->n, nb2 = (size_t)p->nb * p->nb, nv = (size_t)p->nvalid;
  std::vector<float2> htw((size_t)N / 2), hmask(n2);
  for (int j = 0; j < N / 2; j++) {
    const double a = -2.0 * M_PI * (double)j / (double)N;
    htw[j] = make_float2((float)cos(a), (float)sin(a));
  }
  std::vector<unsigned> br((size_t)N);
  for (int i = 0; i < N; i++) br[i] = pyr_brev_host((unsigned)i, p->logn);
  for (int i = 0; i < N; i++)
    for (int q = 0; q < N; q++) {
      const size_t src = (size_t)br[i] * N + br[q];
      const double m = (double)d->submask[src] / (double)N, a = (double)d->halfxy[src];
      hmask[(size_t)i * N + q] = make_float2((float)(m * cos(a)), (float)(m * sin(a)));
    }
  const float one = 1.f, zero = 0.f;
  const size_t fplanes = p->pixel_filter ? (size_t)p->plan.filt_env * n2 : 0;
  bool ok = hipMalloc((void **)&p->mpupil, nn * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->cx, (size_t)p->npts_max * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->cy, (size_t)p->npts_max * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->w, (size_t)p->npts_max * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->ref, 2 * nv * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->hr, (size_t)p->nenv * n2 * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->img, (size_t)p->nenv * nb2 * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->slopes, (size_t)p->nenv * 2 * nv * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->vx, 4 * nv * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&p->vy, 4 * nv * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&p->tw, htw.size() * sizeof(float2)) == hipSuccess &&
            hipMalloc((void **)&p->maskp, n2 * sizeof(float2)) == hipSuccess &&
            hipMalloc((void **)&p->T1, (size_t)p->plan.cap * p->plan.t1_stride * sizeof(float2)) == hipSuccess &&
            hipMalloc((void **)&p->T2, (size_t)p->plan.cap * p->plan.t2_stride * sizeof(float2)) == hipSuccess;
  if (ok && p->pixel_filter)
    ok = hipMalloc((void **)&p->sincar, n2 * sizeof(float)) == hipSuccess &&
         hipMalloc((void **)&p->FA, fplanes * sizeof(float2)) == hipSuccess &&
         hipMalloc((void **)&p->FB, fplanes * sizeof(float2)) == hipSuccess &&
         hipMemcpy(p->sincar, d->sincar, n2 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(p->mpupil, d->mpupil, nn * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->vx, d->validsubsx, 4 * nv * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->vy, d->validsubsy, 4 * nv * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->tw, htw.data(), htw.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->maskp, hmask.data(), n2 * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->w, &one, sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->cx, &zero, sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->cy, &zero, sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(p->ref, 0, 2 * nv * sizeof(float)) == hipSuccess &&
       hipMemset(p->img, 0, (size_t)p->nenv * nb2 * sizeof(float)) == hipSuccess &&
       hipMemset(p->slopes, 0, (size_t)p->nenv * 2 * nv * sizeof(float)) == hipSuccess &&
       hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    aomarl_pyr_destroy(p);
    return fail("pyr_create: device allocation failed (n %d, Nfft %d, %d environments, %d pairs per batch)", d->n, d->Nfft,
                d->nenv, p->plan.cap);
  }
  *out = p;
  return 0;
}

int aomarl_pyr_set_modulation(aomarl_pyr *p, const float *cx, const float *cy, const float *w, int npts, float s_scale) {
  if (!p) return fail("pyr_set_modulation: null object");
  std::string err;
  double wsum = 0;
  if (pyr_validate_modulation(cx, cy, w, npts, p->npts_max, s_scale, &wsum, err)) return fail("%s", err.c_str());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(p->cx, cx, (size_t)npts * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p->cy, cy, (size_t)npts * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p->w, w, (size_t)npts * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  p->npts = npts; p->wsum = wsum; p->s_scale = s_scale;
  return 0;
}

int aomarl_pyr_set_ref(aomarl_pyr *p, const float *ref) {
  if (!p) return fail("pyr_set_ref: null object");
  const size_t bytes = 2 * (size_t)p->nvalid * sizeof(float);
  HIPCHK(hipDeviceSynchronize());
  if (ref) HIPCHK(hipMemcpy(p->ref, ref, bytes, hipMemcpyHostToDevice));
  else HIPCHK(hipMemset(p->ref, 0, bytes));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

template <int LOGN, int CW>
static void pyr_launch_cols(aomarl_pyr *p, int pairs, hipStream_t s) {
  k_pyr_cols<LOGN, CW><<<dim3((1 << LOGN) / CW, pairs), PYR_THREADS, 0, s>>>(p->T1, p->n, p->maskp, p->T2, p->tw);
}

int aomarl_pyr_measure(aomarl_pyr *p, const float *phase, int env_begin, int env_count, int flags, int method,
                       const uint32_t *seeds, uint32_t *frame, float *image, float *slopes, void *stream) {
  if (!p) return fail("pyr_measure: null object");
  if (!phase) return fail("pyr_measure: null phase");
  std::string err;
  if (pyr_validate_measure(p->nenv, env_begin, env_count, flags, method, seeds && frame, p->noise, err))
    return fail("%s", err.c_str());
  hipStream_t s = (hipStream_t)stream;
  const int N = p->N, nt = pyr_line_threads(N);
  int env_b, pts_b;
  pyr_batch(p->plan, p->npts, &env_b, &pts_b);
  const float wscale = 1.f / ((float)N * (float)N);
  for (int e0 = env_begin; e0 < env_begin + env_count; e0 += env_b) {
    const int ne = env_begin + env_count - e0 < env_b ? env_begin + env_count - e0 : env_b;
    for (int k0 = 0; k0 < p->npts; k0 += pts_b) {
      const int nk = p->npts - k0 < pts_b ? p->npts - k0 : pts_b;     // (nk < pts_b only when ne == env_b == 1)
      const int pairs = ne * nk;
      k_pyr_rows<<<dim3(p->n, pairs), nt, 0, s>>>(phase, p->mpupil, p->cx, p->cy, p->n, p->logn, e0, k0, nk, p->k2pi, p->T1,
                                                   p->tw);
      LAUNCHCHK();
      switch (p->logn) {
        case 6: pyr_launch_cols<6, 8>(p, pairs, s); break;
        case 7: pyr_launch_cols<7, 8>(p, pairs, s); break;
        case 8: pyr_launch_cols<8, 8>(p, pairs, s); break;
        case 9: pyr_launch_cols<9, 8>(p, pairs, s); break;
        case 10: pyr_launch_cols<10, 8>(p, pairs, s); break;
        case 11: pyr_launch_cols<11, 4>(p, pairs, s); break;
        default: return fail("pyr_measure: Nfft = %d", N);
      }
      LAUNCHCHK();
      k_pyr_irows<<<dim3(N, ne), nt, 0, s>>>(p->T2, p->logn, e0, k0, nk, p->w, wscale, k0 == 0, p->hr, p->tw);
      LAUNCHCHK();
    }
  }
  if (p->pixel_filter) {
    const float inv_n2 = 1.f / ((float)N * (float)N);
    for (int e0 = env_begin; e0 < env_begin + env_count; e0 += p->plan.filt_env) {
      const int ne = env_begin + env_count - e0 < p->plan.filt_env ? env_begin + env_count - e0 : p->plan.filt_env;
      float *h = p->hr + (size_t)e0 * N * N;
      k_pyr_fft_t<<<dim3(N, ne), nt, 0, s>>>(h, nullptr, p->FA, nullptr, nullptr, 1.f, p->logn, 0, p->tw);
      LAUNCHCHK();
      k_pyr_fft_t<<<dim3(N, ne), nt, 0, s>>>(nullptr, p->FA, p->FB, nullptr, p->sincar, 1.f, p->logn, 0, p->tw);
      LAUNCHCHK();
      k_pyr_fft_t<<<dim3(N, ne), nt, 0, s>>>(nullptr, p->FB, p->FA, nullptr, nullptr, 1.f, p->logn, 1, p->tw);
      LAUNCHCHK();
      k_pyr_fft_t<<<dim3(N, ne), nt, 0, s>>>(nullptr, p->FA, nullptr, h, nullptr, inv_n2, p->logn, 1, p->tw);
      LAUNCHCHK();
    }
  }
  const int noisy = (flags & AOMARL_PYR_NOISE) && p->noise >= 0.f;
  const float scale = (float)((double)p->nphotons / (p->wsum * p->lit));
  const int nb2 = p->nb * p->nb;
  k_pyr_bin<<<dim3((nb2 + PYR_THREADS - 1) / PYR_THREADS, env_count), PYR_THREADS, 0, s>>>(
      p->hr, N, p->nrebin, env_begin, scale, p->noise, noisy, seeds, frame, p->img, image);
  LAUNCHCHK();
  k_pyr_slopes<<<env_count, PYR_THREADS, 0, s>>>(p->img, p->nb, p->nvalid, env_begin, p->vx, p->vy, method, p->thresh,
                                                 p->s_scale, p->ref, p->slopes, slopes, frame, noisy);
  LAUNCHCHK();
  return 0;
}
