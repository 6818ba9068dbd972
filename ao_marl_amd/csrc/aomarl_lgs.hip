// aomarl_lgs.hip -- laser guide star on the Shack-Hartmann sensor (include/aomarl.h: aomarl_lgs_*).  gfx950 only.
// The model is ao_marl_amd/lgs.py (LgsModel, cone_trace_model; float64 NumPy); the reference's host side is
// shesha/init/lgs_init.py, its native side is not in the reference tree.  A translation unit of its own: the cone trace
// reads the context's static description and the state exactly as aomarl_raytrace_wfs does, through aomarl_env_host.h.
// The host half is aomarl_lgs_host.h.
#include "aomarl_env_host.h"
#include "aomarl_trace_dev.h"
#include "aomarl_lgs_host.h"

// =============================================================================================
// k_lgs_trace: k_raytrace<false> with every layer magnified about the pupil centre by delta_l = 1 + dm1[l].
// Shape and arithmetic are k_raytrace's (a workgroup owns 256 consecutive pixels, layers and mirrors summed in a
// register in its order, the mirrors through its own trace_dms, one store per pixel); the only change is the layer
// coordinate, one fused multiply-add on top of k_raytrace's own sum: dm1 = 0 gives that sum unchanged, bit for bit.
// dm1 rides in the kernel's arguments (uniform: scalar registers).
// =============================================================================================
struct LgsCone { float dm1[AOMARL_MAX_LAYERS]; };

__global__ __launch_bounds__(256) void k_lgs_trace(DevSys sys, DevState st, LgsCone cone, int env_begin, int flags) {
  const int nn = sys.n;
  const int e = env_begin + blockIdx.y;
  float *out = st.wfs_phase + (long long)e * nn * nn;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nn * nn) return;
  const int y = p / nn, x = p - y * nn;
  float v = (flags & AOMARL_TRACE_RESET) ? 0.f : out[p];
  if (flags & AOMARL_TRACE_ATMOS) {
    const float c = 0.5f * (float)(nn - 1);
    const float dx = (float)x - c, dy = (float)y - c;      // exact: half-integers below 2^23
    for (int l = 0; l < sys.nlayers; l++) {
      const DevLayer &L = sys.layers[l];
      const float *base = st.screens + (long long)e * sys.screen_stride + L.screen_off;
      const int ox = st.origin[(e * sys.nlayers + l) * 2], oy = st.origin[(e * sys.nlayers + l) * 2 + 1];
      v += bilinear_ring(base, L.dim, ox, oy, __fmaf_rn(cone.dm1[l], dx, (float)x + L.wxo),
                         __fmaf_rn(cone.dm1[l], dy, (float)y + L.wyo));
    }
  }
  if (flags & AOMARL_TRACE_DMS) v = trace_dms<false>(sys, st, e, x, y, v);
  if (flags & AOMARL_TRACE_MASK) v *= sys.mpupil[p];
  out[p] = v;
}

// =============================================================================================
// k_lgs_spot: image, binning, flux, noise, centre of gravity and - ref of one (sub-aperture, environment) per workgroup.
//
// The lag formulation ("Laser guide star"): |fft2(a)|^2 is the DFT of the tile's autocorrelation R(s),
// |s| <= L = PD - 1 per axis (2 PD - 1 < N: no wrap), so the image convolved with the kernel is one pruned DFT of
// G(s) = R(s) Kt(s) over the lags, Kt the kernel's table (aomarl_lgs_host.h: lgs_kernel_table), Hermitian: the half
// sx >= 0 is kept, (2 L + 1) x PD complex numbers = 3968 bytes per sub-aperture, shared by all environments (L2).
//   1  tile: thread (y, x) forms a = mask exp(i (2 pi / lambda phase - halfxy)) into a zero-padded LDS array
//      ap[PD + 2 L][AP_LD] (row y + L, column x) and its conjugate into ac[PD][PD]
//   2  R: lane (t & 31) owns the lag row sy = (t & 31) - L, half wave (t >> 5) the four lags sx0 .. sx0 + 3 of it,
//      sx0 = 4 (t >> 5): PD^2 products per lag, row sums of PD terms added in row order.  Per (y, x) a lane reads ONE new
//      tile element (the window of four slides with x) and the conjugate element every lane shares (a broadcast): two
//      LDS reads for four products.  An 8-byte LDS read is served half a wave at a time: its lanes are the lag rows,
//      AP_LD = 3 PD + 1 is odd, so they fall on 31 distinct 8-byte bank pairs
//   3  G = R Kt into LDS; T(ky, sx) = c_sx sum_sy G(sy, sx) exp(-2 pi i ky sy / N) for the window's rows (c_0 = 1,
//      c_sx = 2: the other half); J(ky, kx) = Re sum_sx T(ky, sx) exp(-2 pi i kx sx / N) for the window's columns
//   4  binning over nrebin x nrebin blocks, the total (a tree in LDS: a fixed order), g = nphotons flux / total, noise,
//      the cube, the three moments (trees), the slopes.
// No atomics; nothing depends on which environments a call covers.
// =============================================================================================
template <int PD> struct LgsLds {
  static constexpr int L = PD - 1, NL = 2 * PD - 1, AP_LD = 3 * PD + 1, AP_ROWS = PD + 2 * (PD - 1);
};

// sum over the workgroup's 256 threads in a fixed order (a tree); every thread gets the total
__device__ __forceinline__ float lgs_block_sum(float v, float *red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int h = LGS_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  return red[0];
}

template <int PD, int N, bool NOISE, bool WRITE_CUBE>
__global__ __launch_bounds__(LGS_THREADS) void k_lgs_spot(const float *__restrict__ phase, const float *__restrict__ mpupil,
                                                           const float *__restrict__ halfxy, const float *__restrict__ flux,
                                                           const int *__restrict__ sub_x0, const int *__restrict__ sub_y0,
                                                           const float2 *__restrict__ kt, const float2 *__restrict__ twid,
                                                           const float *__restrict__ ref, int n, int nvalid, int npix,
                                                           int nrebin, int indi, int env_begin, float k2pi, float nphot,
                                                           float sigma, float cog_offset, float cog_scale,
                                                           const uint32_t *__restrict__ seeds, const uint32_t *__restrict__ frame,
                                                           float *__restrict__ cube, float *__restrict__ slopes) {
  using S = LgsLds<PD>;
  constexpr int L = S::L, NL = S::NL, AP_LD = S::AP_LD, AP_ROWS = S::AP_ROWS;
  constexpr int NG = PD / 4;                     // groups of four lags sx a lag row is cut into
  static_assert(PD * PD <= LGS_THREADS && PD % 4 == 0 && NL <= 32 && 32 * NG <= LGS_THREADS && 2 * PD + 2 < AP_LD,
                "a thread per phase pixel; a lane per lag row, a half wave per group of four lags");
  static_assert(N * N * 4 <= AP_ROWS * AP_LD * 8, "the window's image reuses the padded tile's LDS");
  __shared__ float2 ap[AP_ROWS * AP_LD];         // the padded tile; afterwards the window's image J (floats)
  __shared__ float2 ac[PD * PD];
  __shared__ float2 Gs[NL * PD];
  __shared__ float2 Ts[N * PD];
  __shared__ float2 tw[N];
  __shared__ float Bs[LGS_NPIX_MAX * LGS_NPIX_MAX];
  __shared__ float red[LGS_THREADS];
  const int tid = threadIdx.x, i = blockIdx.x, e = env_begin + blockIdx.y;
  const int W = npix * nrebin, npix2 = npix * npix;

  // ---- 1: the tile
  for (int q = tid; q < AP_ROWS * AP_LD; q += LGS_THREADS) ap[q] = make_float2(0.f, 0.f);
  if (tid < N) tw[tid] = twid[tid];
  __syncthreads();
  if (tid < PD * PD) {
    const int y = tid / PD, x = tid - y * PD;
    const size_t p = (size_t)(sub_y0[i] + y) * n + (size_t)(sub_x0[i] + x);
    const float m = mpupil[p];
    float sn, cs;
    sincosf(k2pi * phase[(size_t)e * n * n + p] - halfxy[tid], &sn, &cs);
    ap[(y + L) * AP_LD + x] = make_float2(m * cs, m * sn);
    ac[tid] = make_float2(m * cs, -(m * sn));
  }
  __syncthreads();

  // ---- 2: the autocorrelation on the half sx >= 0: lane (tid & 31) owns lag row r0 (sy = r0 - L), half wave (tid >> 5)
  // the four lags sx0 .. sx0 + 3 of it, on a window of the tile's row that slides with x
  if ((tid >> 5) < NG && (tid & 31) < NL) {
    const int r0 = tid & 31, sx0 = 4 * (tid >> 5);
    float2 R[4];
#pragma unroll
    for (int j = 0; j < 4; j++) R[j] = make_float2(0.f, 0.f);
#pragma unroll 1
    for (int y = 0; y < PD; y++) {
      const float2 *row = ap + (y + r0) * AP_LD + sx0;    // a(y + sy, x + sx): padded row y + sy + L <= 3 PD - 3, column <= 2 PD + 2
      float2 u0 = row[0], u1 = row[1], u2 = row[2];
      float2 p[4];
#pragma unroll
      for (int j = 0; j < 4; j++) p[j] = make_float2(0.f, 0.f);
#pragma unroll 4
      for (int x = 0; x < PD; x++) {
        const float2 c = ac[y * PD + x], u3 = row[x + 3];
        p[0].x += u0.x * c.x - u0.y * c.y; p[0].y += u0.x * c.y + u0.y * c.x;
        p[1].x += u1.x * c.x - u1.y * c.y; p[1].y += u1.x * c.y + u1.y * c.x;
        p[2].x += u2.x * c.x - u2.y * c.y; p[2].y += u2.x * c.y + u2.y * c.x;
        p[3].x += u3.x * c.x - u3.y * c.y; p[3].y += u3.x * c.y + u3.y * c.x;
        u0 = u1; u1 = u2; u2 = u3;
      }
#pragma unroll
      for (int j = 0; j < 4; j++) { R[j].x += p[j].x; R[j].y += p[j].y; }
    }
    const float2 *k = kt + (size_t)i * NL * PD + r0 * PD + sx0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float2 kj = k[j];
      Gs[r0 * PD + sx0 + j] = make_float2(R[j].x * kj.x - R[j].y * kj.y, R[j].x * kj.y + R[j].y * kj.x);
    }
  }
  __syncthreads();

  // ---- 3: the pruned transform, rows then columns of the window
  for (int q = tid; q < W * PD; q += LGS_THREADS) {
    const int ry = q / PD, s = q - ry * PD, ky = indi + ry;
    float2 a = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int j = 0; j < NL; j++) {
      const float2 g = Gs[j * PD + s], w = tw[(ky * (j - L)) & (N - 1)];
      a.x += g.x * w.x - g.y * w.y;
      a.y += g.x * w.y + g.y * w.x;
    }
    const float c = s == 0 ? 1.f : 2.f;
    Ts[ry * PD + s] = make_float2(c * a.x, c * a.y);
  }
  __syncthreads();
  float *Js = reinterpret_cast<float *>(ap);              // [W][W]
  for (int q = tid; q < W * W; q += LGS_THREADS) {
    const int ry = q / W, rx = q - ry * W, kx = indi + rx;
    float a = 0.f;
#pragma unroll 4
    for (int s = 0; s < PD; s++) {
      const float2 t = Ts[ry * PD + s], w = tw[(kx * s) & (N - 1)];
      a += t.x * w.x - t.y * w.y;
    }
    Js[q] = a;
  }
  __syncthreads();

  // ---- 4: binning, flux, noise, centre of gravity
  float part = 0.f;
  for (int px = tid; px < npix2; px += LGS_THREADS) {
    const int by = px / npix, bx = px - by * npix;
    float s = 0.f;
    for (int yy = 0; yy < nrebin; yy++)
      for (int xx = 0; xx < nrebin; xx++) s += Js[(by * nrebin + yy) * W + bx * nrebin + xx];
    Bs[px] = s;
    part += s;
  }
  const float tot = lgs_block_sum(part, red, tid);
  const float g = tot > 0.f ? nphot * flux[i] / tot : 0.f;
  float m0 = 0.f, mx = 0.f, my = 0.f;
  for (int px = tid; px < npix2; px += LGS_THREADS) {
    const int by = px / npix, bx = px - by * npix;
    float v = Bs[px] * g;
    if (NOISE) v = sh_noise(v, sigma, seeds[e], frame[e], (uint32_t)(i * npix2 + px));
    if (WRITE_CUBE) cube[((size_t)e * nvalid + i) * npix2 + px] = v;
    m0 += v;
    mx += v * (float)bx;
    my += v * (float)by;
  }
  m0 = lgs_block_sum(m0, red, tid);
  mx = lgs_block_sum(mx, red, tid);
  my = lgs_block_sum(my, red, tid);
  if (tid == 0) {
    float *o = slopes + (size_t)e * 2 * nvalid;
    o[i] = (m0 != 0.f ? (mx / m0 - cog_offset) * cog_scale : 0.f) - ref[i];
    o[nvalid + i] = (m0 != 0.f ? (my / m0 - cog_offset) * cog_scale : 0.f) - ref[nvalid + i];
  }
}

// ------------------------------------------------------------------------------------------------- host side
struct aomarl_lgs {
  int nenv, n, pdiam, N, npix, nrebin, nvalid;
  float k2pi, nphotons, noise, cog_offset, cog_scale;
  float *mpupil, *halfxy, *flux, *ref;
  int *sub_x0, *sub_y0;
  float2 *kt, *tw;
};

int aomarl_lgs_destroy(aomarl_lgs *p) {
  if (!p) return 0;
  (void)hipDeviceSynchronize();
  void *q[] = {p->mpupil, p->halfxy, p->flux, p->ref, p->sub_x0, p->sub_y0, p->kt, p->tw};
  for (void *v : q) if (v) (void)hipFree(v);
  delete p;
  return 0;
}

static int lgs_upload_kernels(aomarl_lgs *p, const float *K) {
  const size_t per = (size_t)(2 * p->pdiam - 1) * p->pdiam;
  std::vector<float> tab(2 * per * (size_t)p->nvalid);
  for (int k = 0; k < p->nvalid; k++)
    lgs_kernel_table(K + (size_t)k * p->N * p->N, p->pdiam, p->N, tab.data() + 2 * per * (size_t)k);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(p->kt, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

int aomarl_lgs_create(const aomarl_lgs_desc *d, aomarl_lgs **out) {
  if (!out) return fail("lgs_create: null argument");
  *out = nullptr;
  std::string err;
  if (lgs_validate(d, err)) return fail("%s", err.c_str());
  aomarl_lgs *p = new aomarl_lgs();
  memset((void *)p, 0, sizeof(*p));
  p->nenv = d->nenv; p->n = d->n; p->pdiam = d->pdiam; p->N = d->N; p->npix = d->npix; p->nrebin = d->nrebin;
  p->nvalid = d->nvalid;
  p->k2pi = (float)(2.0 * M_PI / (double)d->lambda_um);
  p->nphotons = d->nphotons; p->noise = d->noise; p->cog_offset = d->cog_offset; p->cog_scale = d->cog_scale;
  const int N = p->N;
  const size_t nn = (size_t)p->n * p->n, pd2 = (size_t)p->pdiam * p->pdiam, nv = (size_t)p->nvalid;
  const size_t per = (size_t)(2 * p->pdiam - 1) * p->pdiam;
  std::vector<float2> htw((size_t)N);
  for (int j = 0; j < N; j++) {
    const double a = -2.0 * M_PI * (double)j / (double)N;
    htw[j] = make_float2((float)cos(a), (float)sin(a));
  }
  bool ok = hipMalloc((void **)&p->mpupil, nn * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->halfxy, pd2 * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->flux, nv * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->ref, 2 * nv * sizeof(float)) == hipSuccess &&
            hipMalloc((void **)&p->sub_x0, nv * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&p->sub_y0, nv * sizeof(int)) == hipSuccess &&
            hipMalloc((void **)&p->kt, nv * per * sizeof(float2)) == hipSuccess &&
            hipMalloc((void **)&p->tw, (size_t)N * sizeof(float2)) == hipSuccess;
  ok = ok && hipMemcpy(p->mpupil, d->mpupil, nn * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->halfxy, d->halfxy, pd2 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->flux, d->flux, nv * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->sub_x0, d->sub_x0, nv * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->sub_y0, d->sub_y0, nv * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(p->tw, htw.data(), (size_t)N * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(p->ref, 0, 2 * nv * sizeof(float)) == hipSuccess;
  if (ok) {                 // the impulse at (N / 2, N / 2): Kt(s) = exp(i pi (sy + sx)) = (-1)^(sy + sx)
    std::vector<float2> imp(nv * per);
    const int L = p->pdiam - 1;
    for (size_t k = 0; k < nv; k++)
      for (int r = 0; r < 2 * L + 1; r++)
        for (int s = 0; s < p->pdiam; s++)
          imp[k * per + (size_t)r * p->pdiam + s] = make_float2(((r - L + s) & 1) ? -1.f : 1.f, 0.f);
    ok = hipMemcpy(p->kt, imp.data(), imp.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess;
  }
  if (!ok) {
    aomarl_lgs_destroy(p);
    return fail("lgs_create: device allocation failed (n %d, %d sub-apertures, %d environments)", d->n, d->nvalid, d->nenv);
  }
  *out = p;
  return 0;
}

int aomarl_lgs_set_kernels(aomarl_lgs *p, const float *K) {
  if (!p) return fail("lgs_set_kernels: null object");
  std::string err;
  if (lgs_validate_kernels(K, p->nvalid, p->N, err)) return fail("%s", err.c_str());
  return lgs_upload_kernels(p, K);
}

int aomarl_lgs_set_ref(aomarl_lgs *p, const float *ref) {
  if (!p) return fail("lgs_set_ref: null object");
  const size_t bytes = 2 * (size_t)p->nvalid * sizeof(float);
  HIPCHK(hipDeviceSynchronize());
  if (ref) HIPCHK(hipMemcpy(p->ref, ref, bytes, hipMemcpyHostToDevice));
  else HIPCHK(hipMemset(p->ref, 0, bytes));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

int aomarl_lgs_trace(aomarl_lgs *p, aomarl_ctx *c, aomarl_state *st, const float *dm1, int nlayers, int b, int n, int flags,
                     void *stream) {
  if (!p || !c || !st) return fail("lgs_trace: null argument");
  const EnvView v = env_view(c);
  if (v.sys.n != p->n) return fail("lgs_trace: the sensor's pupil array is %d wide, the context's %d", p->n, v.sys.n);
  if (st->nenv != p->nenv) return fail("lgs_trace: the sensor has %d environments, the state %d", p->nenv, st->nenv);
  int rc = env_refuse_busy("lgs_trace", c);
  if (rc) return rc;
  std::string err;
  const int known = AOMARL_TRACE_ATMOS | AOMARL_TRACE_DMS | AOMARL_TRACE_RESET | AOMARL_TRACE_MASK;
  if (lgs_validate_trace(dm1, nlayers, v.nlayers, AOMARL_MAX_LAYERS, p->nenv, b, n, flags, known, err))
    return fail("%s", err.c_str());
  rc = env_trace_ready(c, st, b, n, flags, stream);
  if (rc) return rc;
  if (!st->wfs_phase) return fail("lgs_trace needs st->wfs_phase");
  LgsCone cone;
  for (int l = 0; l < AOMARL_MAX_LAYERS; l++) cone.dm1[l] = l < nlayers ? dm1[l] : 0.f;
  const int np = v.sys.n * v.sys.n;
  hipLaunchKernelGGL(k_lgs_trace, dim3((np + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, v.sys, dev_state(st), cone, b,
                     flags);
  LAUNCHCHK();
  return 0;
}

template <int PD, int N, bool NOISE, bool CUBE>
static void lgs_launch_size(aomarl_lgs *p, const LgsPlan &pl, const float *phase, int env_begin, const uint32_t *seeds,
                            const uint32_t *frame, float *image, float *slopes, hipStream_t s) {
  k_lgs_spot<PD, N, NOISE, CUBE><<<dim3(pl.grid_x, pl.grid_y), pl.threads, 0, s>>>(
      phase, p->mpupil, p->halfxy, p->flux, p->sub_x0, p->sub_y0, p->kt, p->tw, p->ref, p->n, p->nvalid, p->npix, p->nrebin,
      pl.indi, env_begin, p->k2pi, p->nphotons, p->noise, p->cog_offset, p->cog_scale, seeds, frame, image, slopes);
}
template <bool NOISE, bool CUBE>
static void lgs_launch_spot(aomarl_lgs *p, const LgsPlan &pl, const float *phase, int env_begin, const uint32_t *seeds,
                            const uint32_t *frame, float *image, float *slopes, hipStream_t s) {
  if (p->pdiam == LGS_PD) lgs_launch_size<LGS_PD, LGS_N, NOISE, CUBE>(p, pl, phase, env_begin, seeds, frame, image, slopes, s);
  else lgs_launch_size<LGS_PD_S, LGS_N_S, NOISE, CUBE>(p, pl, phase, env_begin, seeds, frame, image, slopes, s);   // (create let no other size in)
}

int aomarl_lgs_measure(aomarl_lgs *p, const float *phase, int env_begin, int env_count, int flags, const uint32_t *seeds,
                       uint32_t *frame, float *image, float *slopes, void *stream) {
  if (!p) return fail("lgs_measure: null object");
  if (!phase || !slopes) return fail("lgs_measure: null phase or slopes");
  std::string err;
  if (lgs_validate_measure(p->nenv, env_begin, env_count, flags, seeds && frame, image != nullptr, p->noise, err))
    return fail("%s", err.c_str());
  hipStream_t s = (hipStream_t)stream;
  const bool noisy = (flags & AOMARL_LGS_NOISE) && p->noise >= 0.f, cube = flags & AOMARL_LGS_WRITE_CUBE;
  const LgsPlan pl = lgs_plan(p->nvalid, env_count, p->npix, p->nrebin, p->N, noisy);
  if (noisy && cube) lgs_launch_spot<true, true>(p, pl, phase, env_begin, seeds, frame, image, slopes, s);
  else if (noisy) lgs_launch_spot<true, false>(p, pl, phase, env_begin, seeds, frame, image, slopes, s);
  else if (cube) lgs_launch_spot<false, true>(p, pl, phase, env_begin, seeds, frame, image, slopes, s);
  else lgs_launch_spot<false, false>(p, pl, phase, env_begin, seeds, frame, image, slopes, s);
  LAUNCHCHK();
  return noisy ? launch_inc_u32(frame + env_begin, env_count, s) : 0;
}
