// aomarl_denoise_train.hip -- training step of the WFS-image denoiser: forward with the
// activations kept, mean-squared-error loss, backward through all six layers, Adam.  gfx950 only.
//
// Network (reference: DenoisingAutoencoderCNN2DSingleSubapeture, src/autoencoder/autoencoder_models.py:130-197; its
// training pairs: src/autoencoder/obtain_dataset_autoencoder.py:66-109.  The reference ships no training loop: the
// loss, the mean squared error, and the optimiser, torch.optim.Adam's formula, are this project's choice), per 16x16
// image:
//   conv3x3(1->16)+ReLU+pool2 -> conv3x3(16->32)+ReLU+pool2 -> conv3x3(32->64)+ReLU ->
//   convT4x4s2(64->32)+ReLU -> convT4x4s2(32->16)+ReLU -> convT3x3s1(16->1)
//
// Every product -- forward, input gradient, weight gradient -- is one launch of the learner's grouped GEMM
// (aomarl_gemm_g.h, v_mfma_f32_16x16x4_f32; launched through gemm_g_batched of aomarl_sac.hip, the one unit that
// instantiates it), with gather / fold kernels around it:
//  * activations are channel-last [image][y][x][C], so they ARE row-major GEMM operands;
//  * a convolution is  col = gather(in) [positions][Cin 9],  Z = col W^T + b  with W as the checkpoint holds it
//    ([Cout][Cin 9], k contiguous); its weight gradient is col^T dZ, its input gradient fold(dZ W);
//  * a transposed convolution is  col = in W  with W as the checkpoint holds it ([Cin][Cout k k], n contiguous) and
//    out = fold(col) + b;  backwards dcol = gather(dZ), dW = in^T dcol (already in the checkpoint's layout),
//    d in = dcol W^T under the ReLU mask (the GEMM's mask epilogue);
//  * gather and fold are the same two kernels for all layers (kernel size 3 or 4, stride 1 or 2, padding 1);
//  * the 3x3 single-channel ends (encoder1, decoder3) keep their 9 taps in rows of 12 floats (16-byte rows for the
//    GEMM); the pad columns are zero, get zero gradients and stay zero under Adam.
// Determinism: the weight gradients are split along K = images x positions into slabs of DT_SLAB images (the GEMM's
// group index), each slab writes its own partial, and one kernel adds the slabs in a fixed order; bias gradients and
// the loss alike.  No floating-point atomics anywhere.
// Images beyond `max_batch` are processed in chunks of the workspace's size; a chunk's gradient is added to the
// previous chunks' in the same reduction.  The tail of the last slab is padded with zero images whose output gradient
// is zero.
// Adam keeps its two moments in double and rounds the new weight once: the update is torch.optim.Adam's formula
// evaluated on the fp32 gradients to the last bit of the fp32 weight.
#include "aomarl_host.h"
#include <vector>
#include <math.h>
#include <string.h>

#define DT_SLAB 16          // images per split-K slab of the weight gradients
#define DT_MAXCHUNK 2048    // images per pass over the workspace (about 300 KB of workspace per image)

// flat parameter buffer (floats); gradients and Adam moments use the same offsets
#define DT_W1 0             // [16][12]   encoder1 [16][1][3][3], rows padded 9 -> 12
#define DT_W2 192           // [32][144]
#define DT_W3 4800          // [64][288]
#define DT_W4 23232         // [64][512]  decoder1 [64][32][4][4]
#define DT_W5 56000         // [32][256]  decoder2 [32][16][4][4]
#define DT_W6 64192         // [16][12]   decoder3 [16][1][3][3], rows padded 9 -> 12
#define DT_B1 64384
#define DT_B2 64400
#define DT_B3 64432
#define DT_B4 64496
#define DT_B5 64528
#define DT_B6 64544
#define DT_NPAR 64548       // padded to a multiple of 4

struct DtPtrs { float *w[6], *b[6]; };

// flat index -> (tensor 0..11, index inside the checkpoint's tensor or -1 for a pad column)
__host__ __device__ inline void dt_locate(int i, int *tensor, int *idx) {
  const int off[13] = {DT_W1, DT_W2, DT_W3, DT_W4, DT_W5, DT_W6, DT_B1, DT_B2, DT_B3, DT_B4, DT_B5, DT_B6, DT_B6 + 1};
  int t = 0;
  while (t < 11 && i >= off[t + 1]) t++;
  int j = i - off[t];
  if (i >= DT_B6 + 1) { *tensor = 11; *idx = -1; return; }
  if (t == 0 || t == 5) j = (j % 12) < 9 ? (j / 12) * 9 + (j % 12) : -1;
  *tensor = t; *idx = j;
}

// ---------------------------------------------------------------------------------------------- kernels
// [y][x] tiles -> the network's [x][y]; images past n are zero
__global__ void k_dt_in(const float *__restrict__ noisy, float *__restrict__ xt, int n, int npad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)npad * 256) return;
  const int img = (int)(i >> 8), p = (int)(i & 255);
  xt[i] = img < n ? noisy[(long long)img * 256 + (p & 15) * 16 + (p >> 4)] : 0.f;
}

// col[(img, iy, ix)][c KK + ky ks + kx] = src[img][st iy - 1 + ky][st ix - 1 + kx][c], zero outside the image and in the
// row's pad columns.  Hc: side of the col grid, Hs: side of src.
__global__ void k_dt_gather(const float *__restrict__ src, float *__restrict__ col, long long total, int Hc, int Hs,
                            int Cc, int ks, int st, int ld) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % ld);
  const long long row = i / ld;
  const int KK = ks * ks;
  float v = 0.f;
  if (j < Cc * KK) {
    const int c = j / KK, t = j - c * KK, ky = t / ks, kx = t - ky * ks;
    const int ix = (int)(row % Hc), iy = (int)((row / Hc) % Hc);
    const long long img = row / (Hc * Hc);
    const int y = st * iy - 1 + ky, x = st * ix - 1 + kx;
    if (y >= 0 && y < Hs && x >= 0 && x < Hs) v = src[((img * Hs + y) * Hs + x) * Cc + c];
  }
  col[i] = v;
}

// out[img][oy][ox][c] = act(bias[c] + sum over (ky, kx) of col[(img, (oy + 1 - ky) / st, (ox + 1 - kx) / st)][c KK + ky ks + kx])
// over the taps whose source position exists; taps in a fixed order.
__global__ void k_dt_fold(const float *__restrict__ col, float *__restrict__ out, const float *__restrict__ bias,
                          long long total, int Hc, int Ho, int Cc, int ks, int st, int ld, int relu) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % Cc);
  const long long pos = i / Cc;
  const int ox = (int)(pos % Ho), oy = (int)((pos / Ho) % Ho);
  const long long img = pos / (Ho * Ho);
  const int KK = ks * ks;
  float s = bias ? bias[c] : 0.f;
  for (int ky = 0; ky < ks; ky++) {
    const int ty = oy + 1 - ky;
    if (ty < 0 || ty % st || ty / st >= Hc) continue;
    for (int kx = 0; kx < ks; kx++) {
      const int tx = ox + 1 - kx;
      if (tx < 0 || tx % st || tx / st >= Hc) continue;
      s += col[((img * Hc + ty / st) * Hc + tx / st) * ld + c * KK + ky * ks + kx];
    }
  }
  out[i] = relu ? fmaxf(s, 0.f) : s;
}

// 2x2 max-pool of z [img][2H][2H][C] (already past its ReLU) -> a [img][H][H][C]
__global__ void k_dt_pool(const float *__restrict__ z, float *__restrict__ a, long long total, int H, int Cc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % Cc);
  const long long pos = i / Cc;
  const int x = (int)(pos % H), y = (int)((pos / H) % H);
  const long long img = pos / (H * H);
  const float *p = z + ((img * 2 * H + 2 * y) * 2 * H + 2 * x) * Cc + c;
  a[i] = fmaxf(fmaxf(p[0], p[Cc]), fmaxf(p[2 * H * Cc], p[2 * H * Cc + Cc]));
}

// gradient through max-pool and the ReLU in front of it: the first largest element of the window takes da if it is
// positive (torch picks the first; a window that is all <= 0 passes nothing)
__global__ void k_dt_unpool(const float *__restrict__ z, const float *__restrict__ da, float *__restrict__ dz,
                            long long total, int H, int Cc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % Cc);
  const long long pos = i / Cc;
  const int x = (int)(pos % H), y = (int)((pos / H) % H);
  const long long img = pos / (H * H);
  const long long base = ((img * 2 * H + 2 * y) * 2 * H + 2 * x) * Cc + c;
  const long long o[4] = {0, Cc, (long long)2 * H * Cc, (long long)2 * H * Cc + Cc};
  int best = 0;
  float vb = z[base];
  for (int k = 1; k < 4; k++) {
    const float v = z[base + o[k]];
    if (v > vb) { vb = v; best = k; }
  }
  const float g = vb > 0.f ? da[i] : 0.f;
  for (int k = 0; k < 4; k++) dz[base + o[k]] = k == best ? g : 0.f;
}

// out (net orientation) -> d loss / d out in place, one block per slab of DT_SLAB images; the slab's sum of squares in
// double.  clean: [y][x] tiles.
__global__ __launch_bounds__(256) void k_dt_loss(float *__restrict__ out, const float *__restrict__ clean, int n,
                                                 float scale, double *__restrict__ part) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int k = 0; k < DT_SLAB; k++) {
    const int img = blockIdx.x * DT_SLAB + k;
    const long long i = (long long)img * 256 + tid;
    float d = 0.f;
    if (img < n) d = out[i] - clean[(long long)img * 256 + (tid & 15) * 16 + (tid >> 4)];
    out[i] = d * scale;
    s += (double)d * (double)d;
  }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

__global__ void k_dt_loss_final(const double *__restrict__ part, int nslab, int first, double inv_count,
                                double *__restrict__ acc, float *__restrict__ loss_out) {
  if (threadIdx.x || blockIdx.x) return;
  double s = first ? 0.0 : *acc;
  for (int g = 0; g < nslab; g++) s += part[g];
  *acc = s;
  if (loss_out) *loss_out = (float)(s * inv_count);
}

// bias gradient of one slab: part[g][c] = sum over the slab's rows of dz[row][c]; Cc divides 256
__global__ __launch_bounds__(256) void k_dt_colsum(const float *__restrict__ dz, int rows, int Cc, float *__restrict__ part,
                                                   long long spart) {
  __shared__ float red[256];
  const int tid = threadIdx.x, c = tid % Cc, rl = tid / Cc, nrl = 256 / Cc;
  const float *p = dz + (long long)blockIdx.x * rows * Cc + c;
  float s = 0.f;
  for (int r = rl; r < rows; r += nrl) s += p[(long long)r * Cc];
  red[tid] = s;
  __syncthreads();
  if (tid < Cc) {
    float t = 0.f;
    for (int r = 0; r < nrl; r++) t += red[r * Cc + tid];
    part[(long long)blockIdx.x * spart + tid] = t;
  }
}

// grad[i] (+)= the slabs' partials in slab order.  The convolutions' partials are [Cin 9][Cout] (col^T dZ): transposed here.
__global__ void k_dt_reduce(const float *__restrict__ part, int nslab, int accumulate, float *__restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= DT_NPAR) return;
  int src = i;
  if (i < DT_W2) src = DT_W1 + (i % 12) * 16 + i / 12;
  else if (i < DT_W3) src = DT_W2 + ((i - DT_W2) % 144) * 32 + (i - DT_W2) / 144;
  else if (i < DT_W4) src = DT_W3 + ((i - DT_W3) % 288) * 64 + (i - DT_W3) / 288;
  float s = accumulate ? grad[i] : 0.f;
  if (i <= DT_B6)
    for (int g = 0; g < nslab; g++) s += part[(long long)g * DT_NPAR + src];
  grad[i] = s;
}

// torch.optim.Adam (no weight decay, no amsgrad): m, v in double, one rounding of the new weight.  eps > 0 (create
// refuses anything else), so the pad columns and the buffer's tail, whose g = m = v = 0 for ever, get 0 / eps = 0.
__global__ void k_dt_adam(float *__restrict__ par, const float *__restrict__ grad, double *__restrict__ m,
                          double *__restrict__ v, double lr, double b1, double b2, double eps, double bc1, double bc2s) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= DT_NPAR) return;
  const double g = (double)grad[i];
  const double mi = b1 * m[i] + (1.0 - b1) * g, vi = b2 * v[i] + (1.0 - b2) * g * g;
  m[i] = mi; v[i] = vi;
  const double denom = sqrt(vi) / bc2s + eps;
  par[i] = (float)((double)par[i] - (lr / bc1) * (mi / denom));
}

// flat buffer -> the twelve tensors of the checkpoint
__global__ void k_dt_unpack(const float *__restrict__ flat, DtPtrs out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > DT_B6) return;
  int t, j;
  dt_locate(i, &t, &j);
  if (j < 0) return;
  float *dst = t < 6 ? out.w[t] : out.b[t - 6];
  if (dst) dst[j] = flat[i];
}

// ------------------------------------------------------------------------------------------- host side
struct aomarl_denoiser_trainer {
  int chunk;                     // images per pass (a multiple of DT_SLAB)
  long long steps;
  double lr, b1, b2, eps;
  float *par, *grad, *part, *ws;
  double *m, *v, *lossp, *lossacc;
  // workspace, per chunk (floats per image in brackets)
  float *xt, *col1, *z1, *a1, *col2, *z2, *a2, *col3, *a3, *cd1, *a4, *cd2, *a5, *cd3, *out;
  float *da5, *da4, *da3, *da2, *dz2, *da1, *dz1;
};

int aomarl_denoiser_trainer_destroy(aomarl_denoiser_trainer *tr) {
  if (!tr) return 0;
  void *p[] = {tr->par, tr->grad, tr->part, tr->ws, tr->m, tr->v, tr->lossp, tr->lossacc};
  for (void *q : p) if (q) (void)hipFree(q);
  delete tr;
  return 0;
}

int aomarl_denoiser_trainer_create(const float *const *wt, const float *const *bs, double lr, double beta1, double beta2,
                                   double eps, int max_batch, aomarl_denoiser_trainer **out) {
  if (!wt || !bs || !out) return fail("denoiser_trainer_create: null argument");
  for (int i = 0; i < 6; i++) if (!wt[i] || !bs[i]) return fail("denoiser_trainer_create: null layer %d", i);
  if (max_batch < 1) return fail("denoiser_trainer_create: max_batch %d", max_batch);
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0))
    return fail("denoiser_trainer_create: lr %g betas (%g, %g) eps %g", lr, beta1, beta2, eps);
  aomarl_denoiser_trainer *tr = new aomarl_denoiser_trainer();
  memset(tr, 0, sizeof(*tr));
  tr->lr = lr; tr->b1 = beta1; tr->b2 = beta2; tr->eps = eps;
  const int want = (max_batch + DT_SLAB - 1) / DT_SLAB * DT_SLAB;
  tr->chunk = want < DT_MAXCHUNK ? want : DT_MAXCHUNK;
  const int nslab = tr->chunk / DT_SLAB;
  const size_t per[] = {256, 256 * 12, 256 * 16, 64 * 16, 64 * 144, 64 * 32, 16 * 32, 16 * 288, 16 * 64, 16 * 512, 64 * 32,
                        64 * 256, 256 * 16, 256 * 12, 256, 256 * 16, 64 * 32, 16 * 64, 16 * 32, 64 * 32, 64 * 16, 256 * 16};
  float **dst[] = {&tr->xt, &tr->col1, &tr->z1, &tr->a1, &tr->col2, &tr->z2, &tr->a2, &tr->col3, &tr->a3, &tr->cd1, &tr->a4,
                   &tr->cd2, &tr->a5, &tr->cd3, &tr->out, &tr->da5, &tr->da4, &tr->da3, &tr->da2, &tr->dz2, &tr->da1,
                   &tr->dz1};
  size_t total = 0;
  for (size_t f : per) total += f;
  std::vector<float> flat(DT_NPAR, 0.f);
  const int nw[6] = {16 * 9, 32 * 144, 64 * 288, 64 * 512, 32 * 256, 16 * 9}, nb[6] = {16, 32, 64, 32, 16, 1};
  for (int i = 0; i <= DT_B6; i++) {
    int t, j;
    dt_locate(i, &t, &j);
    if (j < 0) continue;
    if (j >= (t < 6 ? nw[t] : nb[t - 6])) { delete tr; return fail("denoiser_trainer_create: layout"); }
    flat[i] = t < 6 ? wt[t][j] : bs[t - 6][j];
  }
  bool ok = hipMalloc((void **)&tr->par, DT_NPAR * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&tr->grad, DT_NPAR * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&tr->m, DT_NPAR * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&tr->v, DT_NPAR * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&tr->part, (size_t)nslab * DT_NPAR * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&tr->lossp, (size_t)nslab * sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&tr->lossacc, sizeof(double)) == hipSuccess &&
            hipMalloc((void **)&tr->ws, total * tr->chunk * sizeof(float)) == hipSuccess;
  ok = ok && hipMemcpy(tr->par, flat.data(), DT_NPAR * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(tr->grad, 0, DT_NPAR * sizeof(float)) == hipSuccess &&
       hipMemset(tr->m, 0, DT_NPAR * sizeof(double)) == hipSuccess &&
       hipMemset(tr->v, 0, DT_NPAR * sizeof(double)) == hipSuccess &&
       hipMemset(tr->part, 0, (size_t)nslab * DT_NPAR * sizeof(float)) == hipSuccess &&
       hipMemset(tr->lossacc, 0, sizeof(double)) == hipSuccess &&
       hipMemset(tr->ws, 0, total * tr->chunk * sizeof(float)) == hipSuccess;
  if (!ok) {
    const size_t mb = total * tr->chunk * sizeof(float) >> 20;
    aomarl_denoiser_trainer_destroy(tr);
    return fail("denoiser_trainer_create: device allocation failed (%zu MB of workspace)", mb);
  }
  float *p = tr->ws;
  for (size_t i = 0; i < sizeof(per) / sizeof(per[0]); i++) { *dst[i] = p; p += per[i] * tr->chunk; }
  *out = tr;
  return 0;
}

static int dt_gemm(int groups, bool ak, bool bk, int M, int N, int K, const float *A, int lda, long long sA,
                   const float *B, int ldb, long long sB, float *C, int ldc, long long sC, const float *bias, int relu,
                   const float *mask, int ldm, hipStream_t s) {
  if (gemm_g_batched(groups, ak, bk, M, N, K, A, lda, sA, B, ldb, sB, bias, 0, C, ldc, sC, relu, mask, ldm, s))
    return fail("denoiser_trainer: GEMM launch failed (%d x %d x %d)", M, N, K);
  g_arith[AR_GEMM_F32]++;
  return 0;
}

static inline unsigned dt_blocks(long long total) { return (unsigned)((total + 255) / 256); }

// one chunk: n real images (padded to whole slabs); gradient into tr->grad (added to it when `accumulate`)
static int dt_chunk(aomarl_denoiser_trainer *tr, const float *noisy, const float *clean, int n, long long ntotal,
                    int accumulate, float *loss_out, hipStream_t s) {
  const int np = (n + DT_SLAB - 1) / DT_SLAB * DT_SLAB, nslab = np / DT_SLAB;
  const long long P256 = (long long)np * 256, P64 = (long long)np * 64, P16 = (long long)np * 16;
  const float *W1 = tr->par + DT_W1, *W2 = tr->par + DT_W2, *W3 = tr->par + DT_W3, *W4 = tr->par + DT_W4,
              *W5 = tr->par + DT_W5, *W6 = tr->par + DT_W6;
#define DT_K(kern, total, ...)                                                                     \
  do {                                                                                             \
    hipLaunchKernelGGL(kern, dim3(dt_blocks(total)), dim3(256), 0, s, __VA_ARGS__);                \
    LAUNCHCHK();                                                                                   \
  } while (0)
#define DT_G(...) do { if (dt_gemm(__VA_ARGS__, s)) return 1; } while (0)
  // ---------------- forward
  DT_K(k_dt_in, P256, noisy, tr->xt, n, np);
  DT_K(k_dt_gather, P256 * 12, tr->xt, tr->col1, P256 * 12, 16, 16, 1, 3, 1, 12);
  DT_G(1, true, true, (int)P256, 16, 12, tr->col1, 12, 0, W1, 12, 0, tr->z1, 16, 0, tr->par + DT_B1, 1, nullptr, 0);
  DT_K(k_dt_pool, P64 * 16, tr->z1, tr->a1, P64 * 16, 8, 16);
  DT_K(k_dt_gather, P64 * 144, tr->a1, tr->col2, P64 * 144, 8, 8, 16, 3, 1, 144);
  DT_G(1, true, true, (int)P64, 32, 144, tr->col2, 144, 0, W2, 144, 0, tr->z2, 32, 0, tr->par + DT_B2, 1, nullptr, 0);
  DT_K(k_dt_pool, P16 * 32, tr->z2, tr->a2, P16 * 32, 4, 32);
  DT_K(k_dt_gather, P16 * 288, tr->a2, tr->col3, P16 * 288, 4, 4, 32, 3, 1, 288);
  DT_G(1, true, true, (int)P16, 64, 288, tr->col3, 288, 0, W3, 288, 0, tr->a3, 64, 0, tr->par + DT_B3, 1, nullptr, 0);
  DT_G(1, true, false, (int)P16, 512, 64, tr->a3, 64, 0, W4, 512, 0, tr->cd1, 512, 0, nullptr, 0, nullptr, 0);
  DT_K(k_dt_fold, P64 * 32, tr->cd1, tr->a4, tr->par + DT_B4, P64 * 32, 4, 8, 32, 4, 2, 512, 1);
  DT_G(1, true, false, (int)P64, 256, 32, tr->a4, 32, 0, W5, 256, 0, tr->cd2, 256, 0, nullptr, 0, nullptr, 0);
  DT_K(k_dt_fold, P256 * 16, tr->cd2, tr->a5, tr->par + DT_B5, P256 * 16, 8, 16, 16, 4, 2, 256, 1);
  DT_G(1, true, false, (int)P256, 12, 16, tr->a5, 16, 0, W6, 12, 0, tr->cd3, 12, 0, nullptr, 0, nullptr, 0);
  DT_K(k_dt_fold, P256, tr->cd3, tr->out, tr->par + DT_B6, P256, 16, 16, 1, 3, 1, 12, 0);
  // ---------------- loss, d out
  hipLaunchKernelGGL(k_dt_loss, dim3(nslab), dim3(256), 0, s, tr->out, clean, n, (float)(2.0 / ((double)ntotal * 256.0)),
                     tr->lossp);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_dt_loss_final, dim3(1), dim3(64), 0, s, tr->lossp, nslab, accumulate ? 0 : 1,
                     1.0 / ((double)ntotal * 256.0), tr->lossacc, loss_out);
  LAUNCHCHK();
  // ---------------- backward.  Slab g of a weight gradient goes to part[g][layer offset ...]
  float *part = tr->part;
  const long long sP = DT_NPAR;
  auto colsum = [&](const float *dz, int rows, int Cc, int off) {
    hipLaunchKernelGGL(k_dt_colsum, dim3(nslab), dim3(256), 0, s, dz, rows, Cc, part + off, sP);
    return hipGetLastError() == hipSuccess ? 0 : fail("denoiser_trainer: launch failed");
  };
  const int R256 = DT_SLAB * 256, R64 = DT_SLAB * 64, R16 = DT_SLAB * 16;
  // decoder3
  if (colsum(tr->out, R256, 1, DT_B6)) return 1;
  DT_K(k_dt_gather, P256 * 12, tr->out, tr->cd3, P256 * 12, 16, 16, 1, 3, 1, 12);
  DT_G(nslab, false, false, 16, 12, R256, tr->a5, 16, (long long)R256 * 16, tr->cd3, 12, (long long)R256 * 12,
       part + DT_W6, 12, sP, nullptr, 0, nullptr, 0);
  DT_G(1, true, true, (int)P256, 16, 12, tr->cd3, 12, 0, W6, 12, 0, tr->da5, 16, 0, nullptr, 0, tr->a5, 16);
  // decoder2
  if (colsum(tr->da5, R256, 16, DT_B5)) return 1;
  DT_K(k_dt_gather, P64 * 256, tr->da5, tr->cd2, P64 * 256, 8, 16, 16, 4, 2, 256);
  DT_G(nslab, false, false, 32, 256, R64, tr->a4, 32, (long long)R64 * 32, tr->cd2, 256, (long long)R64 * 256,
       part + DT_W5, 256, sP, nullptr, 0, nullptr, 0);
  DT_G(1, true, true, (int)P64, 32, 256, tr->cd2, 256, 0, W5, 256, 0, tr->da4, 32, 0, nullptr, 0, tr->a4, 32);
  // decoder1
  if (colsum(tr->da4, R64, 32, DT_B4)) return 1;
  DT_K(k_dt_gather, P16 * 512, tr->da4, tr->cd1, P16 * 512, 4, 8, 32, 4, 2, 512);
  DT_G(nslab, false, false, 64, 512, R16, tr->a3, 64, (long long)R16 * 64, tr->cd1, 512, (long long)R16 * 512,
       part + DT_W4, 512, sP, nullptr, 0, nullptr, 0);
  DT_G(1, true, true, (int)P16, 64, 512, tr->cd1, 512, 0, W4, 512, 0, tr->da3, 64, 0, nullptr, 0, tr->a3, 64);
  // encoder3 (da3 is d Z3: the mask epilogue applied the ReLU)
  if (colsum(tr->da3, R16, 64, DT_B3)) return 1;
  DT_G(nslab, false, false, 288, 64, R16, tr->col3, 288, (long long)R16 * 288, tr->da3, 64, (long long)R16 * 64,
       part + DT_W3, 64, sP, nullptr, 0, nullptr, 0);
  DT_G(1, true, false, (int)P16, 288, 64, tr->da3, 64, 0, W3, 288, 0, tr->col3, 288, 0, nullptr, 0, nullptr, 0);
  DT_K(k_dt_fold, P16 * 32, tr->col3, tr->da2, (const float *)nullptr, P16 * 32, 4, 4, 32, 3, 1, 288, 0);
  DT_K(k_dt_unpool, P16 * 32, tr->z2, tr->da2, tr->dz2, P16 * 32, 4, 32);
  // encoder2
  if (colsum(tr->dz2, R64, 32, DT_B2)) return 1;
  DT_G(nslab, false, false, 144, 32, R64, tr->col2, 144, (long long)R64 * 144, tr->dz2, 32, (long long)R64 * 32,
       part + DT_W2, 32, sP, nullptr, 0, nullptr, 0);
  DT_G(1, true, false, (int)P64, 144, 32, tr->dz2, 32, 0, W2, 144, 0, tr->col2, 144, 0, nullptr, 0, nullptr, 0);
  DT_K(k_dt_fold, P64 * 16, tr->col2, tr->da1, (const float *)nullptr, P64 * 16, 8, 8, 16, 3, 1, 144, 0);
  DT_K(k_dt_unpool, P64 * 16, tr->z1, tr->da1, tr->dz1, P64 * 16, 8, 16);
  // encoder1
  if (colsum(tr->dz1, R256, 16, DT_B1)) return 1;
  DT_G(nslab, false, false, 12, 16, R256, tr->col1, 12, (long long)R256 * 12, tr->dz1, 16, (long long)R256 * 16,
       part + DT_W1, 16, sP, nullptr, 0, nullptr, 0);
  DT_K(k_dt_reduce, DT_NPAR, part, nslab, accumulate, tr->grad);
#undef DT_K
#undef DT_G
  return 0;
}

static int dt_grads(aomarl_denoiser_trainer *tr, const float *noisy, const float *clean, long long nimg, float *loss_out,
                    hipStream_t s) {
  if (!tr || !noisy || !clean) return fail("denoiser_trainer: null argument");
  if (nimg < 1 || nimg > 0x7fffffffLL / 4096) return fail("denoiser_trainer: %lld images", nimg);
  for (long long i0 = 0; i0 < nimg; i0 += tr->chunk) {
    const int n = (int)(nimg - i0 < tr->chunk ? nimg - i0 : tr->chunk);
    if (dt_chunk(tr, noisy + i0 * 256, clean + i0 * 256, n, nimg, i0 > 0, loss_out, s)) return 1;
  }
  return 0;
}

static int dt_unpack(const float *flat, float *const *w, float *const *b, hipStream_t s) {
  DtPtrs o;
  for (int i = 0; i < 6; i++) { o.w[i] = w ? w[i] : nullptr; o.b[i] = b ? b[i] : nullptr; }
  hipLaunchKernelGGL(k_dt_unpack, dim3(dt_blocks(DT_NPAR)), dim3(256), 0, s, flat, o);
  LAUNCHCHK();
  return 0;
}

int aomarl_denoiser_trainer_grads(aomarl_denoiser_trainer *tr, const float *noisy, const float *clean, long long nimg,
                                  float *const *grads_w, float *const *grads_b, float *loss_out, void *stream) {
  if (dt_grads(tr, noisy, clean, nimg, loss_out, (hipStream_t)stream)) return 1;
  return dt_unpack(tr->grad, grads_w, grads_b, (hipStream_t)stream);
}

int aomarl_denoiser_trainer_step(aomarl_denoiser_trainer *tr, const float *noisy, const float *clean, long long nimg,
                                 float *loss_out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dt_grads(tr, noisy, clean, nimg, loss_out, s)) return 1;
  tr->steps++;
  const double bc1 = 1.0 - pow(tr->b1, (double)tr->steps), bc2 = 1.0 - pow(tr->b2, (double)tr->steps);
  hipLaunchKernelGGL(k_dt_adam, dim3(dt_blocks(DT_NPAR)), dim3(256), 0, s, tr->par, tr->grad, tr->m, tr->v, tr->lr, tr->b1,
                     tr->b2, tr->eps, bc1, sqrt(bc2));
  LAUNCHCHK();
  return 0;
}

int aomarl_denoiser_trainer_get(aomarl_denoiser_trainer *tr, float *const *weights, float *const *biases, void *stream) {
  if (!tr || !weights || !biases) return fail("denoiser_trainer_get: null argument");
  return dt_unpack(tr->par, weights, biases, (hipStream_t)stream);
}
