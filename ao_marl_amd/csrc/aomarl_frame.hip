// aomarl_frame.hip -- the one-pass frame kernel of the environment, k_frame_wave, and its launcher: a translation unit
// of its own (its 48 instantiations are most of the library's compile time).  It sees the device description
// (aomarl_dev.h) and the launch arguments (aomarl_frame_host.h), not the context.
#include "aomarl_frame_host.h"
#include "aomarl_spot_dev.h"

// =============================================================================================
// ONE-PASS FRAME KERNEL: WFS spot images + COG  and  science-path PSF rows from ONE pass over the
// phase.  The sub-aperture tiles (16 x 16 phase pixels starting at pad + 16 k of the WFS grid) are
// exactly the 16 x 16 tiles of the pupil grid the target sees, at the same screen / DM pixels, so
// every phase pixel is read once and feeds both paths: per tile 48 MFMAs (pruned spot DFT) if it
// is a valid sub-aperture + 16 MFMAs (PSF row DFT).
//
// Work split: ONE WAVE = ONE (environment, stripe of 16 pupil rows); it walks the tiles of the
// stripe left to right, so its 16 PSF rows stay in its accumulators (no cross-wave reduction) and
// its per-environment constants are scalars.  The 4 waves of a block work on the same stripe of
// 4 consecutive environments: the data shared by all environments (tip-tilt planes, pupil mask
// rows, PSF twiddles) is fetched at about the same time by the 4 waves and hits in the L1.
// The pupil mask comes as 16-bit rows; tiles outside the pupil are skipped.
//
// Lane (q, c) owns the pixels (y = c, x = 4q .. 4q+3) of the tile -- the accumulator layout of a
// 16x16x4 MFMA whose M index is x and N index is y, so the stack-array DM phase can be produced IN
// PLACE on the matrix cores (OTF = true): with the separable influence profile u and the command
// lattice C of the environment,
//     S[x][y] = sum_j u(x - X_j) sum_i C[j][i] u(y - Y_i)
// is two tiny GEMMs (lattice nodes that reach a tile: 4 .. 8 per axis): stage A over i (A operand
// = lattice patch from LDS, B operand = profile column, a per-lane constant), stage B over j
// (A operand = profile, B operand = the accumulator registers of stage A, whose row order
// j(m) = (m >> 2) + 4 (m & 3) makes register s the K-slice of MFMA s).  2 MFMAs for <= 4 nodes
// (NB = 1), 4 for <= 8 (NB = 2): the DM shape of the pupil never exists in memory.
// LDS tiles are stored transposed ([x][y], row stride 20 floats): writes by (q, c) and the
// operand reads (x = 4q + s, y = c) both touch 32 distinct banks per half wave.
// =============================================================================================
#define FW_LD 20
// tile_info bits: [15:0] sub-aperture index, 16 lit, 17 every pixel lit, 18 has a valid sub-aperture
#define FW_LIT 0x10000
#define FW_FULL 0x20000
#define FW_SUB 0x40000
// science-path phase in revolutions for v_sin / v_cos, unreduced.  The ISA text gives the instructions a
// valid input domain of [-256, 256] revolutions; measured on gfx950 (tests/test_gpu_phase_range.py), they
// reduce far past it: phases of +-660 um (1320 sensor / 400 science revolutions) give the slopes, spots
// and Strehl ratios of the same frame without the whole-period offset to fp32 round-off of the phase
// itself.  The explicit round-and-subtract the WFS path keeps (its fused multiply-subtract saves one
// rounding, which the 2e-5 image tolerance needs) is therefore dropped here.
__device__ __forceinline__ float sci_rev(float ph, float inv_lambda) { return ph * inv_lambda; }

// Uniform tables that nothing writes during a launch, read through the CONSTANT address space: the compiler
// then uses scalar loads (s_load, counted by lgkmcnt) instead of a vector load + v_readfirstlane.  It matters
// for the per-tile walk of the lit-tile list: vector loads return in order, so waiting for the list entry --
// the newest load in flight -- made every wave wait for ALL its prefetched tile loads at the top of each
// iteration (s_waitcnt vmcnt(0)): the software pipeline of the frame kernel collapsed to one stage.
typedef const int __attribute__((address_space(4))) *const_int_p;
typedef const float __attribute__((address_space(4))) *const_float_p;

template <int NL, bool OTF>
struct FrameRaw {
  float L[NL][4];
  float P[OTF ? 1 : 4], T[8];
  unsigned mrow;      // 16-bit mask row of the tile (this lane's row)
  float F;
  f4u SH;             // this wave's quarter of the tile's environment-independent data
  float4 CS;          // the PSF operand of the lane (pair walk: read out of the block's slot by the caller, like T)
};

// Both arithmetics share one skeleton.  The data of a tile that does not depend on the environment
// (tip-tilt planes: 2 x 16 bytes per lane; PSF twiddle operand: 16 bytes per lane) is fetched once per
// BLOCK -- each of the 4 waves loads one quarter a tile ahead, parks it in a double-buffered LDS slot, one
// barrier per lit tile -- instead of once per wave from L2, and two tiles of loads are in flight per wave.
// HP = false (default, the reference's arithmetic): fp32 operands on v_mfma_f32_16x16x4_f32.  Lane (q, c)
// owns the pixels (y = c, x = 4q + s): with K step s of an MFMA taking x = 4q + s from K lane q, the lane's
// own four amplitudes ARE the A operands of the first DFT stage and of the PSF rows, and the accumulator
// registers of stage 1 the B operands of stage 2: no amplitude tile ever goes through LDS.
// HP = true (fast mode): the same products on split-fp16 MFMAs (hi + lo operand pairs).
//
// Science path: R[y][kx] = sum_x a(y, x) exp(-2 pi i kx X / Npsf), X = 16 t + x, kx in [-8, 8).  cos is
// even and sin odd in kx, so the 16 columns of ONE real operand  [cos k X (k = 1..8) | sin k X (k = 1..8)]
// serve every kx != 0:  PA = a_r . [C|S],  PB = a_i . [C|S]  (8 fp32 MFMAs per tile instead of 16 for the
// plain complex product; 4 instead of 8 split-fp16 ones), accumulated over the whole stripe and combined
// once at its end:  kx = +k: (PA_C + PB_S, PB_C - PA_S);  kx = -k: (PA_C - PB_S, PB_C + PA_S).  The
// kx = 0 column is the plain row sum of the amplitudes: 8 vector adds per tile.
template <int NL, int NB, bool OTF, bool NOISE, bool WRITE_CUBE, bool HP>
// 3 waves per SIMD (<= 168 VGPRs): the kernel is bound by issue slots, not by latency -- a fourth wave (<= 128
// registers, 8 of them spilled) made it slower
// Layer rows of a PAIR of adjacent tiles as whole 128-byte pieces, straight into LDS (the stack-array-from-
// voltages instantiations).  A load instruction that covers 16 rows x 64 B (the compute layout: lane (q, c) = row c,
// pixels 4q .. 4q + 3) makes the memory pipeline handle every 128-byte line twice, half a line at a time; as
// 8 rows x 128 contiguous bytes the same bytes arrive 25 % faster (tools/dmabench.hip: 3.9 -> 4.9 TB/s on this access
// pattern alone).  (HBM-side bytes do not go down -- a 128-byte run at a 4-byte-aligned start straddles two lines 7
// times out of 8: 1.6 GB per launch against 1.47 -- the number of requests does.)  The pieces are written by
// buffer_load_dwordx4 ... lds -- no vector registers in flight -- into the wave's own LDS image: per layer two blocks of
// 8 rows x 8 chunks of 16 bytes in LANE order (what that instruction can write), the second block 128 bytes further,
// the chunk a lane fetches XOR-ed with its row (lane = 8 row + (chunk ^ row)): the compute layout's ds_read_b128
// (row c, chunk 4 h + q of tile h) then finds its 16 lanes in 16 different bank groups.
#define FWD_BLK 1152                       // bytes from block 0 to block 1 of a layer image (FWD_IMG bytes: aomarl_dev.h)
// (the slopes-only fp32 instantiations are held to 128 registers, the budget of four waves: beside a product's wave
// and a scatter / gather block two frame waves have 256 of the SIMD's 512 -- what runs at a time is set by the LDS request)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((OTF && !HP && !NOISE && !WRITE_CUBE) ? 4 : 3, (OTF && !HP && !NOISE && !WRITE_CUBE) ? 4 : 3)))
void k_frame_wave(DevSys sys, DevState st, int env_begin,
                                                    int env_count, int do_cog,
                                                    float *__restrict__ TR,
                                                    float *__restrict__ TPART, int nblk) {
  extern __shared__ float smem[];
  const int pd = sys.pupdiam, ntl = sys.ntiles;
  const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, c = lane & 15;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // slopes only, fp32: the moments as quadratic forms of the field (spot_qf_moments): no transform, no Cc / Ss, no
  // twiddle table -- the lane's constants come from sys.qf_tab
  constexpr bool QF = OTF && !HP && !NOISE && !WRITE_CUBE;
  constexpr bool DMA = OTF;                                  // the pair walk
  const FrameLds lds = frame_lds(QF, OTF, NL, NB, sys.otf_latw, ntl);
  char *const lds0 = reinterpret_cast<char *>(smem);
  float2 *sTw = reinterpret_cast<float2 *>(lds0);                // [128] WFS twiddles (none in the slopes-only instantiation)
  float *lat_all = reinterpret_cast<float *>(lds0 + lds.lat);    // [4 waves][4 NB][latw]
  float4 *shb = reinterpret_cast<float4 *>(lds0 + lds.slots);    // the block's shared-data slots
  char *dimg = lds0 + lds.img + (DMA ? wv * NL * FWD_IMG : 0);   // this wave's layer images
  // slopes-only fp32 instantiation: the moments of the stripe's sub-apertures, [tile][s0, ty, tx, -] per wave,
  // turned into slopes once per stripe by lane = tile (the per-tile finish was a dozen instructions on ONE lane)
  float4 *qmom = reinterpret_cast<float4 *>(lds0 + lds.qmom) + wv * ntl;
  const int dbg = do_cog >> 8;                               // development switches (kbench)
  do_cog &= 1;
  // blocks are dispatched x-fastest: x = group of 4 environments, y = rank of the stripe by
  // decreasing number of lit tiles -- the longest stripes start first and the launch ends on the
  // shortest ones (longest-processing-time order: smaller tail)
  const int r = sys.stripe_order[blockIdx.y];                // stripe: pupil rows 16 r .. 16 r + 15
  const int el = 4 * blockIdx.x + wv;                        // environment of this wave
  if constexpr (!QF) {
    if (tid < 128) {
      float sn, cs;
      sincospif((float)tid * (1.0f / 64.0f), &sn, &cs);
      sTw[tid] = make_float2(cs, sn);
    }
    __syncthreads();
  }
  const bool active = el < env_count;          // a wave past the last environment repeats it (see the tile)
  const int e = env_begin + (active ? el : env_count - 1);
  float Cc[4] = {0.f, 0.f, 0.f, 0.f}, Ss[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (!QF) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const float2 w = sTw[((4 * q + s) * (2 * c + 1)) & 127];
      Cc[s] = w.x; Ss[s] = w.y;
    }
  }
  SpotTwH twh;
  if (HP) twh = spot_tw_h(Cc, Ss);
  SpotQf qfk;
  if constexpr (QF) {
    const float4 ka = reinterpret_cast<const float4 *>(sys.qf_tab)[2 * lane], kb = reinterpret_cast<const float4 *>(sys.qf_tab)[2 * lane + 1];
    qfk.h = f32x4{ka.x, ka.y, ka.z, ka.w};
    qfk.ky = f32x2{kb.x, kb.y}; qfk.kx = kb.z;
  }
  // shared loads: wave 0 / 1: the two 16-byte halves of the lane's tip-tilt pairs, wave 2 (and 3, a
  // duplicate that hits in the L1): the PSF operand of the lane, [t][64] x 16 B
  unsigned shstep;
  const int y = 16 * r + c;                                  // pupil row of this lane
  // ---- per-environment constants (target-path offsets; the WFS sees the same pixels).
  // Every load address is  scalar base (advances with the tile)  +  per-lane byte offset (fixed
  // for the stripe): rows carry RING_PAD = 16 mirror columns, so the 16-byte load of a lane may
  // start up to 12 floats past the scalar wrap point without wrapping itself.
  // Loads go through buffer descriptors (scalar base + 32-bit per-lane offset + scalar offset of
  // the tile): no 64-bit address arithmetic on the vector unit, no address registers.
  const char *layb[NL];
  __amdgpu_buffer_rsrc_t lrs[NL];
  unsigned lpxs[NL], ldim[NL], lvo[NL];
#pragma unroll
  for (int l = 0; l < NL; l++) {
    const DevLayer &L = sys.layers[l];
    layb[l] = reinterpret_cast<const char *>(st.screens + (long long)e * sys.screen_stride + L.screen_off);
    lrs[l] = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(layb[l]), 0,
                                               4 * L.dim * (L.dim + RING_PAD), 0x00020000);
    ldim[l] = (unsigned)L.dim;
    int px = L.tox + st.origin[(e * sys.nlayers + l) * 2]; px -= (px >= L.dim) ? L.dim : 0;
    int py = L.toy + st.origin[(e * sys.nlayers + l) * 2 + 1]; py -= (py >= L.dim) ? L.dim : 0;
    lpxs[l] = (unsigned)px;
    unsigned pr = (unsigned)y + (unsigned)py; pr = min(pr, pr - ldim[l]);
    lvo[l] = 4u * (pr * (ldim[l] + RING_PAD) + 4u * (unsigned)q);
  }
  const DevDm &D0 = sys.dms[0], &D1 = sys.dms[1];
  const float *pzt = st.dm_shape + (long long)e * sys.shape_stride + D0.shape_off;
  const float *ttslot = st.dm_shape + (long long)e * sys.shape_stride + D1.shape_off;
  const float c0 = ttslot[0], c1 = ttslot[1];
  const int half = pd / 2;
  const unsigned pvo = 4u * ((unsigned)(y + D0.toy) * (unsigned)D0.dim + (unsigned)D0.tox + 4u * (unsigned)q);
  // tip-tilt planes re-arranged per 4 pixels of a pupil row: [x0 x1 x2 x3 | y0 y1 y2 y3] (sys.tt_pk), so that a
  // lane's two 16-byte halves are the x-plane and the y-plane values of its 4 pixels (pairs for packed FMAs)
  const unsigned tvo = 32u * ((unsigned)y * (unsigned)(pd >> 2) + (unsigned)q);
  const unsigned mvo = 2u * (unsigned)y * (unsigned)ntl;
  const char *pztb = reinterpret_cast<const char *>(pzt);
  const char *ttb = reinterpret_cast<const char *>(sys.tt_pk);
  const char *mkb = reinterpret_cast<const char *>(sys.tile_mask);
  // (selected with scalar selects, not in two branches: the descriptor must stay provably wave-uniform, or
  // every load through it is wrapped in a waterfall loop)
  const bool sh_tt = wv < 2;
  const void *shbase = sh_tt ? static_cast<const void *>(ttb) : (HP ? sys.psf_tw_h : sys.psf_tw_f);
  const __amdgpu_buffer_rsrc_t shrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void *>(shbase), 0, sh_tt ? 8 * pd * pd : ntl * 1024, 0x00020000);
  const unsigned shvo = sh_tt ? tvo + 16u * (unsigned)wv : 16u * (unsigned)lane;
  shstep = sh_tt ? 7u : 10u;          // log2 of the bytes per tile (a shift stays on the scalar unit; the
                                      // compiler turns a multiplication into a VECTOR mul24 + waterfall loop)
  // pivot of the variance sums: phase at the grid centre (ttslot[2]: stack-array value there)
  float pivot;
  {
    float v = OTF ? ttslot[2] : pzt[(half + D0.toy) * D0.dim + half + D0.tox];
    const float2 f = reinterpret_cast<const float2 *>(D1.influ)[(half + D1.toy) * D1.dim + half + D1.tox];
    v += c0 * f.x + c1 * f.y;
#pragma unroll
    for (int l = 0; l < NL; l++) {
      const DevLayer &L = sys.layers[l];
      int py = L.toy + st.origin[(e * sys.nlayers + l) * 2 + 1]; py -= (py >= L.dim) ? L.dim : 0;
      unsigned pyc = (unsigned)(half + py); pyc = min(pyc, pyc - ldim[l]);
      unsigned pxc = (unsigned)half + lpxs[l]; pxc = min(pxc, pxc - ldim[l]);
      v += reinterpret_cast<const float *>(layb[l])[pyc * (ldim[l] + RING_PAD) + pxc];
    }
    pivot = v;
  }
  // ---- on-the-fly stack-array DM: profile operands + the lattice rows of this stripe in LDS
  float Pxr[NB], Pyr[NB];
  const int jm = (c >> 2) + 4 * (c & 3);
  const bool jm_ok = jm < 4 * NB;
  const int latw = sys.otf_latw, tpn = sys.otf_tpn;
  float *lat = lat_all + wv * (4 * NB * latw);
  if (OTF) {
#pragma unroll
    for (int s = 0; s < NB; s++) {
      const int ax = sys.otf_xoff + c - D0.pitch * (q + 4 * s);
      const int ay = sys.otf_yoff + c - D0.pitch * (q + 4 * s);
      Pxr[s] = (ax >= 0 && ax < D0.ss) ? D0.prof[ax] : 0.f;
      Pyr[s] = (ay >= 0 && ay < D0.ss) ? D0.prof[ay] : 0.f;
    }
    const float *volt = st.voltage + (long long)e * st.ld_actu + D0.com_off;
    // (row by row, a lane per column: the flat index over rows x columns cost an integer division per element, a
    // hundred vector instructions at the head of every wave)
    for (int i = 0; i < 4 * NB; i++) {
      const int gy = sys.otf_gy0 + r * tpn + i;
      for (int jj = lane; jj < latw; jj += 64) {
        const int gx = sys.otf_gx0 + jj;
        float v = 0.f;
        if (gx >= 0 && gx < D0.gw && gy >= 0 && gy < D0.gh) {
          const int a = D0.grid[gy * D0.gw + gx];
          if (a >= 0) v = volt[a];
        }
        lat[i * latw + jj] = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  const float *latq = lat + (jm_ok ? jm : 0);
  const float wfs_il = sys.wfs_inv_lambda, tar_il = sys.tar_inv_lambda;
  const f32x4 Z4 = opaque_zero4();
  f32x4 PA = {0.f, 0.f, 0.f, 0.f}, PB = {0.f, 0.f, 0.f, 0.f};     // a_r . [C|S], a_i . [C|S] of the stripe
  float R0r = 0.f, R0i = 0.f;                                     // kx = 0: row sums of this lane's 4 columns
  float sd = 0.f, sd2 = 0.f, sm = 0.f;
  int nlit = 0;
  // packed-fp32 form of the tile's vector arithmetic (fp32 arithmetic with the stack-array DM evaluated in here:
  // the instantiations the loop launches).  The pivot of the variance sums goes into the C operand of the
  // lattice product, so the phase of the tile comes out as phase - pivot: a piston, invisible to |.|^2 of either
  // path, and the variance sums take the phase as it stands.
  constexpr bool PK = OTF && !HP;
  const f32x4 NP4 = {-pivot, -pivot, -pivot, -pivot};
  const f32x2 c0c0 = {c0, c0}, c1c1 = {c1, c1};
  const f32x2 wil2 = {sys.wfs_inv_lambda, sys.wfs_inv_lambda}, til2 = {sys.tar_inv_lambda, sys.tar_inv_lambda};
  f32x2 sdp = {0.f, 0.f}, sd2p = {0.f, 0.f}, R0rp = {0.f, 0.f}, R0ip = {0.f, 0.f};
  int nfull = 0;

  const const_float_p cflux = (const_float_p)(unsigned long long)sys.flux;
  // Loads of one lit tile.  UNCONDITIONAL: the loops below walk the compact list of this stripe's
  // lit tiles (sys.lit_info), so no load sits under a branch and the prefetch registers need no
  // copies where control flow joins (those copies were 9 % of the vector instructions).
  auto fetch = [&](int info, FrameRaw<NL, OTF> &raw) {
    const int t = (info >> 24) & 0x7F;
    {   // consumed first (slot write at the top of the tile): issued first, so that waiting for it never
        // waits for the layer loads behind it (vector loads return in order)
      const f32x4 v4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(shrs, shvo, (unsigned)t << shstep, 0));
#pragma unroll
      for (int j = 0; j < 4; j++) raw.SH.v[j] = v4[j];
    }
    raw.mrow = *reinterpret_cast<const uint16_t *>(mkb + 2u * (unsigned)t + mvo);
#pragma unroll
    for (int l = 0; l < NL; l++) {
      unsigned sx = 16u * (unsigned)t + lpxs[l]; sx -= (sx >= ldim[l]) ? ldim[l] : 0u;   // scalar
      // (whole-vector bit cast: a per-element __builtin_bit_cast of the result is narrowed to ONE dword
      // load by this compiler, ROCm 7.2)
      const f32x4 v4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(lrs[l], lvo[l], 4u * sx, 0));
#pragma unroll
      for (int j = 0; j < 4; j++) raw.L[l][j] = v4[j];
    }
    if (!OTF) {
      const f4u p4 = *reinterpret_cast<const f4u *>(pztb + 64u * (unsigned)t + pvo);
#pragma unroll
      for (int j = 0; j < 4; j++) raw.P[OTF ? 0 : j] = p4.v[j];
    }
    raw.F = cflux[info & 0xFFFF];                            // scalar load; no sub-aperture: index 0, unused
  };

  // one lit tile: consume `cur`, then issue the loads of the tile `infon` describes into `nxt`
  // (dma_slot != nullptr: the pair walk below -- cur.L / mrow / F are filled in by the caller, the block's shared data
  // of this tile is already in `dma_slot`, nothing is fetched in here)
  // mode 0: the tile of the per-tile walk; 2: the same without the fetch of a further tile (the last tiles of a stripe)
  auto tile = [&](int info, int infon, FrameRaw<NL, OTF> &cur, FrameRaw<NL, OTF> &nxt, auto mode_tag, float4 *dma_slot) {
    constexpr bool DM = decltype(mode_tag)::value == 1;
    constexpr bool NOFETCH = decltype(mode_tag)::value != 0;
    const int t = (info >> 24) & 0x7F;
    // ---- stack-array DM phase of the tile on the matrix cores (independent of the loads)
    f32x4 S = PK ? NP4 : Z4;
    if (OTF) {
      f32x4 U = Z4;
#pragma unroll
      for (int kb = 0; kb < NB; kb++) {
        const float a = latq[(q + 4 * kb) * latw + t * tpn];
        U = mfma16(jm_ok ? a : 0.f, Pyr[kb], U);
      }
#pragma unroll
      for (int s = 0; s < NB; s++) S = mfma16(Pxr[s], U[s], S);
    }
    const float flux_i = cur.F;
    // environment-independent data of the tile through the block's LDS slot
    float4 *slot = DM ? dma_slot : shb + (nlit & 1) * 256;
    if constexpr (!DM) {
      nlit++;
      slot[wv * 64 + lane] = make_float4(cur.SH.v[0], cur.SH.v[1], cur.SH.v[2], cur.SH.v[3]);
      __syncthreads();
    }
    const float4 t0 = slot[lane], t1 = slot[64 + lane];
    cur.T[0] = t0.x; cur.T[1] = t0.y; cur.T[2] = t0.z; cur.T[3] = t0.w;
    cur.T[4] = t1.x; cur.T[5] = t1.y; cur.T[6] = t1.z; cur.T[7] = t1.w;
    cur.CS = slot[128 + lane];
    const float4 csP = cur.CS;                     // HP: [hi | lo] halfs; fp32: the 4 K steps
    // (a wave without an environment of its own -- env_count not a multiple of 4 -- repeats the block's last
    // one: same loads, same arithmetic, same values stored twice.  No branch on `active` in here: a join behind
    // a branch that issues loads makes the compiler wait for ALL loads in flight, vmcnt(0), on both sides)
    // ---- phase of the 4 pixels, both complex amplitudes (registers)
    float wr[4], wi[4], ar[4], ai[4];
    if constexpr (PK) {
      // phase - pivot of the 4 pixels as two pairs: S + c0 X + c1 Y + layers (10 packed instructions)
      const f32x2 X01 = {cur.T[0], cur.T[1]}, X23 = {cur.T[2], cur.T[3]};
      const f32x2 Y01 = {cur.T[4], cur.T[5]}, Y23 = {cur.T[6], cur.T[7]};
      PK_GUARD_MFMA();
      f32x2 p01 = pk_fma_s(X01, c0c0, pk_lo(S)), p23 = pk_fma_s(X23, c0c0, pk_hi(S));
      p01 = pk_fma_s(Y01, c1c1, p01); p23 = pk_fma_s(Y23, c1c1, p23);
#pragma unroll
      for (int l = 0; l < NL; l++) {
        const f32x2 l01 = {cur.L[l][0], cur.L[l][1]}, l23 = {cur.L[l][2], cur.L[l][3]};
        p01 = pk_add(p01, l01); p23 = pk_add(p23, l23);
      }
      if (info & FW_FULL) {
        const f32x2 t01 = pk_mul_s(p01, wil2), t23 = pk_mul_s(p23, wil2);
        const f32x2 b01 = pk_mul_s(p01, til2), b23 = pk_mul_s(p23, til2);
        if constexpr (QF) {
          // Slopes only: the sensor's phase goes to v_sin / v_cos as it stands, in revolutions, like the science
          // path's (the instructions reduce the argument themselves, also past the ISA's +-256: see sci_rev; an 8 m
          // pupil sees a few tens of revolutions at 0.5 um).  The explicit round-and-subtract below keeps one rounding less in the REDUCED argument -- what
          // the 2e-5 image tolerance of the image-producing instantiations needs; the centre of gravity does not see
          // it (6e-8 x |revolutions| of phase per pixel, unbiased: 1e-7 pixel of centroid), and the reference itself
          // takes cos / sin of the unreduced float phase.  Six vector instructions less per tile.
          sdp += p01; sd2p = __builtin_elementwise_fma(p01, p01, sd2p);
          sdp += p23; sd2p = __builtin_elementwise_fma(p23, p23, sd2p);
          wr[0] = __builtin_amdgcn_cosf(t01.x); wi[0] = __builtin_amdgcn_sinf(t01.x);
          wr[1] = __builtin_amdgcn_cosf(t01.y); wi[1] = __builtin_amdgcn_sinf(t01.y);
          wr[2] = __builtin_amdgcn_cosf(t23.x); wi[2] = __builtin_amdgcn_sinf(t23.x);
          wr[3] = __builtin_amdgcn_cosf(t23.y); wi[3] = __builtin_amdgcn_sinf(t23.y);
        } else {
        // (plain vector arithmetic, not the in-place asm forms: behind an asm the allocator copied both accumulators
        // into fresh registers in front of the full tile and back at the join with the partial tile's path -- four
        // v_mov_b64 per full tile; the compiler packs these itself)
        sdp += p01; sd2p = __builtin_elementwise_fma(p01, p01, sd2p);
        const f32x2 r01 = {rintf(t01.x), rintf(t01.y)}, r23 = {rintf(t23.x), rintf(t23.y)};
        sdp += p23; sd2p = __builtin_elementwise_fma(p23, p23, sd2p);
        const f32x2 a01 = pk_fma_nc_s(p01, wil2, r01), a23 = pk_fma_nc_s(p23, wil2, r23);
        wr[0] = __builtin_amdgcn_cosf(a01.x); wi[0] = __builtin_amdgcn_sinf(a01.x);
        wr[1] = __builtin_amdgcn_cosf(a01.y); wi[1] = __builtin_amdgcn_sinf(a01.y);
        wr[2] = __builtin_amdgcn_cosf(a23.x); wi[2] = __builtin_amdgcn_sinf(a23.x);
        wr[3] = __builtin_amdgcn_cosf(a23.y); wi[3] = __builtin_amdgcn_sinf(a23.y);
        }
        ar[0] = __builtin_amdgcn_cosf(b01.x); ai[0] = __builtin_amdgcn_sinf(b01.x);
        ar[1] = __builtin_amdgcn_cosf(b01.y); ai[1] = __builtin_amdgcn_sinf(b01.y);
        ar[2] = __builtin_amdgcn_cosf(b23.x); ai[2] = __builtin_amdgcn_sinf(b23.x);
        ar[3] = __builtin_amdgcn_cosf(b23.y); ai[3] = __builtin_amdgcn_sinf(b23.y);
        nfull++;
      } else {
        const float ph4[4] = {p01.x, p01.y, p23.x, p23.y};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float ph = ph4[j];
          const bool m = (cur.mrow >> (4 * q + j)) & 1u;
          float a_ = ph * wfs_il; a_ -= rintf(a_);
          const float b_ = sci_rev(ph, tar_il);
          wr[j] = m ? __builtin_amdgcn_cosf(a_) : 0.f; wi[j] = m ? __builtin_amdgcn_sinf(a_) : 0.f;
          ar[j] = m ? __builtin_amdgcn_cosf(b_) : 0.f; ai[j] = m ? __builtin_amdgcn_sinf(b_) : 0.f;
          const float d = m ? ph : 0.f;
          sd += d; sd2 += d * d; sm += m ? 1.f : 0.f;
        }
      }
    } else if (info & FW_FULL) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float ph = (OTF ? S[j] : cur.P[OTF ? 0 : j]) + (c0 * cur.T[j] + c1 * cur.T[4 + j]);
#pragma unroll
        for (int l = 0; l < NL; l++) ph += cur.L[l][j];
        float a_ = ph * wfs_il; a_ -= rintf(a_);
        const float b_ = sci_rev(ph, tar_il);
        wr[j] = __builtin_amdgcn_cosf(a_); wi[j] = __builtin_amdgcn_sinf(a_);
        ar[j] = __builtin_amdgcn_cosf(b_); ai[j] = __builtin_amdgcn_sinf(b_);
        const float d = ph - pivot;
        sd += d; sd2 += d * d;
      }
      sm += 4.f;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float ph = (OTF ? S[j] : cur.P[OTF ? 0 : j]) + (c0 * cur.T[j] + c1 * cur.T[4 + j]);
#pragma unroll
        for (int l = 0; l < NL; l++) ph += cur.L[l][j];
        const bool m = (cur.mrow >> (4 * q + j)) & 1u;
        float a_ = ph * wfs_il; a_ -= rintf(a_);
        const float b_ = sci_rev(ph, tar_il);
        wr[j] = m ? __builtin_amdgcn_cosf(a_) : 0.f; wi[j] = m ? __builtin_amdgcn_sinf(a_) : 0.f;
        ar[j] = m ? __builtin_amdgcn_cosf(b_) : 0.f; ai[j] = m ? __builtin_amdgcn_sinf(b_) : 0.f;
        const float d = m ? ph - pivot : 0.f;
        sd += d; sd2 += d * d; sm += m ? 1.f : 0.f;
      }
    }
    if constexpr (!NOFETCH) fetch(infon, nxt);               // these loads fly during the MFMAs
    // ---- science path (see the kernel's header)
    if (!(dbg & 2)) {
      if constexpr (PK) {
        const f32x2 ar01 = {ar[0], ar[1]}, ar23 = {ar[2], ar[3]}, ai01 = {ai[0], ai[1]}, ai23 = {ai[2], ai[3]};
        PK_GUARD_TRANS();
        const f32x2 sr_ = pk_add(ar01, ar23), si_ = pk_add(ai01, ai23);
        pk_acc_add(R0rp, sr_); pk_acc_add(R0ip, si_);
        PK_END_TO_MFMA();
      } else {
        R0r += (ar[0] + ar[1]) + (ar[2] + ar[3]);
        R0i += (ai[0] + ai[1]) + (ai[2] + ai[3]);
      }
      if (HP) {
        const hx8 csH = __builtin_bit_cast(hx8, csP);
        hx8 arH, arL, aiH, aiL;
        dup_hl(ar[0], ar[1], ar[2], ar[3], arH, arL);
        dup_hl(ai[0], ai[1], ai[2], ai[3], aiH, aiL);
        PA = mfma_h(arH, csH, PA); PA = mfma_h(arL, csH, PA);
        PB = mfma_h(aiH, csH, PB); PB = mfma_h(aiL, csH, PB);
      } else {
        PA = mfma16(ar[0], csP.x, PA); PB = mfma16(ai[0], csP.x, PB);
        PA = mfma16(ar[1], csP.y, PA); PB = mfma16(ai[1], csP.y, PB);
        PA = mfma16(ar[2], csP.z, PA); PB = mfma16(ai[2], csP.z, PB);
        PA = mfma16(ar[3], csP.w, PA); PB = mfma16(ai[3], csP.w, PB);
      }
    }
    // ---- WFS path (valid sub-apertures only; wave-uniform branch)
    if ((info & FW_SUB) && !(dbg & 1)) {
      if (HP) {
        float v[2][2][2];
        spot_dft_h_v(twh, wr, wi, Z4, v);
        spot_finish_v<NOISE, WRITE_CUBE>(sys, st, e, info & 0xFFFF, lane, v, do_cog, flux_i);
      } else if (!NOISE && !WRITE_CUBE) {
        if constexpr (QF) {
          const float z = spot_qf_moments(qfk, wr, wi, Z4);
          if (c == 0 && q < 3) reinterpret_cast<float *>(qmom + t)[q] = z;     // lanes 0, 16, 32: the three row totals
        } else spot_cog_f32(sys, st, e, info & 0xFFFF, lane, Cc, Ss, wr, wi, do_cog, Z4);
      } else {
        spot_core<NOISE, WRITE_CUBE>(sys, st, e, info & 0xFFFF, lane, Cc, Ss, wr, wi, do_cog, flux_i, Z4);
      }
    }
  };

  // Two fully lit sub-aperture tiles of a pair as ONE instruction block (the slopes-only fp32 instantiations; about nine
  // pairs in ten at 40 x 40).  tile() is a strictly serial chain -- lattice product U, S behind it, the wait states in
  // front of the phase arithmetic, slot reads, phases, transcendentals, PSF rows, stage 1 and stage 2 of the moments,
  // wait states, ten dependent cross-lane steps, one LDS write -- and two calls in a row put tile B's independent work
  // behind tile A's last reduction.  Here the two chains take turns, so that a matrix instruction never reads what one
  // of the two matrix instructions in front of it wrote (the lattice and B's last two products apart: two chains each),
  // one guard serves both tiles' phases, B's transcendentals sit between A's matrix instructions, and A's moments,
  // reduction and LDS write between B's stage-1 instructions.  Every value comes from the same operations in the same
  // order as in tile(): PA / PB take A's four K steps before B's, the packed sums A's terms before B's -- the same
  // bits.  FW_SEQ pins the order written here (a scheduling barrier: the compiler's own interleave of independent
  // matrix chains needed long s_nops of its own).
#define FW_SEQ() __builtin_amdgcn_sched_barrier(0)
  // where a lane puts a tile's row total: lanes 0, 16, 32 into the three moments, every other lane into the fourth word
  // of the tile's entry, which nothing reads.  No branch in the block: with a divergent one at its end the compiler
  // merged it with tile()'s and ran the two paths of the pair walk as one sequence, one's registers live through the other.
  float *const qsel = reinterpret_cast<float *>(qmom) + ((c == 0 && q < 3) ? q : 3);
  [[maybe_unused]] auto pair_block = [&](int ia, int ib, const FrameRaw<NL, OTF> &a, const FrameRaw<NL, OTF> &b, const float4 *sl) {
    static_assert(!QF || PK, "the pair block is the packed fp32 form");
    const int ta = (ia >> 24) & 0x7F, tb = (ib >> 24) & 0x7F;
    // ---- A's tip-tilt planes out of its slot: in flight during the lattice products
    const float4 xa = sl[lane], ya = sl[64 + lane];
    // ---- lattice: U_A, U_B, S_A, S_B
    f32x4 UA = Z4, UB = Z4;
#pragma unroll
    for (int kb = 0; kb < NB; kb++) {
      const float la = latq[(q + 4 * kb) * latw + ta * tpn], lb = latq[(q + 4 * kb) * latw + tb * tpn];
      UA = mfma16(jm_ok ? la : 0.f, Pyr[kb], UA);
      UB = mfma16(jm_ok ? lb : 0.f, Pyr[kb], UB);
    }
    f32x4 SA = NP4, SB = NP4;
#pragma unroll
    for (int s = 0; s < NB; s++) {
      SA = mfma16(Pxr[s], UA[s], SA);
      SB = mfma16(Pxr[s], UB[s], SB);
    }
    // (matrix instructions have no side effect the compiler would order against the packed groups: without this it
    // moves B's two down in front of B's phases)
    asm volatile("" : "+v"(SA), "+v"(SB));
    // ---- phases behind ONE guard.  B's tip-tilt planes are read where A's have been used up (the phases are where
    // the block holds the most registers); A's layer sums cover the reads
    const f32x2 XA01 = {xa.x, xa.y}, XA23 = {xa.z, xa.w}, YA01 = {ya.x, ya.y}, YA23 = {ya.z, ya.w};
    PK_GUARD_MFMA();
    f32x2 a01 = pk_fma_s(XA01, c0c0, pk_lo(SA)), a23 = pk_fma_s(XA23, c0c0, pk_hi(SA));
    a01 = pk_fma_s(YA01, c1c1, a01); a23 = pk_fma_s(YA23, c1c1, a23);
    FW_SEQ();
    const float4 xb = sl[256 + lane], yb = sl[320 + lane];
    FW_SEQ();
#pragma unroll
    for (int l = 0; l < NL; l++) {
      const f32x2 la01 = {a.L[l][0], a.L[l][1]}, la23 = {a.L[l][2], a.L[l][3]};
      a01 = pk_add(a01, la01); a23 = pk_add(a23, la23);
    }
    const f32x2 XB01 = {xb.x, xb.y}, XB23 = {xb.z, xb.w}, YB01 = {yb.x, yb.y}, YB23 = {yb.z, yb.w};
    f32x2 b01 = pk_fma_s(XB01, c0c0, pk_lo(SB)), b23 = pk_fma_s(XB23, c0c0, pk_hi(SB));
    b01 = pk_fma_s(YB01, c1c1, b01); b23 = pk_fma_s(YB23, c1c1, b23);
#pragma unroll
    for (int l = 0; l < NL; l++) {
      const f32x2 lb01 = {b.L[l][0], b.L[l][1]}, lb23 = {b.L[l][2], b.L[l][3]};
      b01 = pk_add(b01, lb01); b23 = pk_add(b23, lb23);
    }
    const f32x2 wa01 = pk_mul_s(a01, wil2), wa23 = pk_mul_s(a23, wil2), wb01 = pk_mul_s(b01, wil2), wb23 = pk_mul_s(b23, wil2);
    const f32x2 ta01 = pk_mul_s(a01, til2), ta23 = pk_mul_s(a23, til2), tb01 = pk_mul_s(b01, til2), tb23 = pk_mul_s(b23, til2);
    // variance sums: A's four terms, then B's (in-place forms: plain arithmetic is placed by the compiler where it
    // likes, here behind the whole block, and the four phases then hold eight registers all the way)
    pk_acc_add(sdp, a01); pk_acc_fma(sd2p, a01, a01);
    pk_acc_add(sdp, a23); pk_acc_fma(sd2p, a23, a23);
    pk_acc_add(sdp, b01); pk_acc_fma(sd2p, b01, b01);
    pk_acc_add(sdp, b23); pk_acc_fma(sd2p, b23, b23);
    FW_SEQ();
    nfull += 2;
    // the PSF operands of both tiles: read behind the phases, which hold the most registers, in flight during A's
    // transcendentals
    const float4 ca = sl[128 + lane], cb = sl[384 + lane];
    // ---- A's sixteen transcendentals and its kx = 0 row sums.  B's sixteen go between the matrix instructions of A
    // below, one pair behind each pair of those (all 32 up here held 134 registers; the limit is 128)
    float wrA[4], wiA[4], arA[4], aiA[4], wrB[4], wiB[4], arB[4], aiB[4];
    const float wa[4] = {wa01.x, wa01.y, wa23.x, wa23.y}, sa[4] = {ta01.x, ta01.y, ta23.x, ta23.y};
    const float wb[4] = {wb01.x, wb01.y, wb23.x, wb23.y}, sb[4] = {tb01.x, tb01.y, tb23.x, tb23.y};
#pragma unroll
    for (int j = 0; j < 4; j++) { wrA[j] = __builtin_amdgcn_cosf(wa[j]); wiA[j] = __builtin_amdgcn_sinf(wa[j]); }
#pragma unroll
    for (int j = 0; j < 4; j++) { arA[j] = __builtin_amdgcn_cosf(sa[j]); aiA[j] = __builtin_amdgcn_sinf(sa[j]); }
    {
      const f32x2 ar01 = {arA[0], arA[1]}, ar23 = {arA[2], arA[3]}, ai01 = {aiA[0], aiA[1]}, ai23 = {aiA[2], aiA[3]};
      PK_GUARD_TRANS();
      const f32x2 sra = pk_add(ar01, ar23), sia = pk_add(ai01, ai23);
      pk_acc_add(R0rp, sra); pk_acc_add(R0ip, sia);
      PK_END_TO_MFMA();
    }
    // ---- matrix stream.  K step k of A's PSF rows beside stage 1 of A's moments: four accumulators in turn
    const float csa[4] = {ca.x, ca.y, ca.z, ca.w}, csb[4] = {cb.x, cb.y, cb.z, cb.w};
    f32x4 DrA = Z4, DiA = Z4;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      PA = mfma16(arA[k], csa[k], PA); PB = mfma16(aiA[k], csa[k], PB);
      wrB[k] = __builtin_amdgcn_cosf(wb[k]); wiB[k] = __builtin_amdgcn_sinf(wb[k]);
      FW_SEQ();
      DrA = mfma16(wrA[k], qfk.h[k], DrA); DiA = mfma16(wiA[k], qfk.h[k], DiA);
      arB[k] = __builtin_amdgcn_cosf(sb[k]); aiB[k] = __builtin_amdgcn_sinf(sb[k]);
      FW_SEQ();
    }
    {   // B's kx = 0 row sums, behind A's in R0rp / R0ip
      const f32x2 br01 = {arB[0], arB[1]}, br23 = {arB[2], arB[3]}, bi01 = {aiB[0], aiB[1]}, bi23 = {aiB[2], aiB[3]};
      PK_GUARD_TRANS();
      const f32x2 srb = pk_add(br01, br23), sib = pk_add(bi01, bi23);
      pk_acc_add(R0rp, srb); pk_acc_add(R0ip, sib);
      PK_END_TO_MFMA();
    }
    // B's PSF rows beside stage 2 of A: four accumulators in turn (with stage 1 of B in here as well -- six -- the block
    // needs more than 128 registers)
    f32x4 PrA = Z4, PiA = Z4;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      PA = mfma16(arB[k], csb[k], PA); PB = mfma16(aiB[k], csb[k], PB);
      FW_SEQ();
      PrA = mfma16(qfk.h[k], DrA[k], PrA); PiA = mfma16(qfk.h[k], DiA[k], PiA);
      FW_SEQ();
    }
    // stage 1 of B, with A's moments, reduction and LDS write between its steps
    f32x4 DrB = mfma16(wrB[0], qfk.h[0], Z4), DiB = mfma16(wiB[0], qfk.h[0], Z4);
    FW_SEQ();
    asm volatile("s_nop 7");                     // with the two instructions above: 10 wait states behind PiA
    const QfTerms mA = qf_products(qfk, PrA, PiA);
    DrB = mfma16(wrB[1], qfk.h[1], DrB); DiB = mfma16(wiB[1], qfk.h[1], DiB);
    FW_SEQ();
    float zA = qf_fold_rows(qfk, mA);
    FW_SEQ();
    DrB = mfma16(wrB[2], qfk.h[2], DrB); DiB = mfma16(wiB[2], qfk.h[2], DiB);
    FW_SEQ();
    zA = qf_fold_lanes(zA);
    FW_SEQ();
    DrB = mfma16(wrB[3], qfk.h[3], DrB); DiB = mfma16(wiB[3], qfk.h[3], DiB);
    FW_SEQ();
    qsel[4 * ta] = zA;
    // stage 2 of B and its moments
    f32x4 PrB = Z4, PiB = Z4;
#pragma unroll
    for (int k = 0; k < 4; k++) { PrB = mfma16(qfk.h[k], DrB[k], PrB); PiB = mfma16(qfk.h[k], DiB[k], PiB); }
    PK_GUARD_MFMA();
    const float zB = qf_fold_lanes(qf_fold_rows(qfk, qf_products(qfk, PrB, PiB)));
    qsel[4 * tb] = zB;
  };

  if constexpr (DMA) {
    // ---- the stripe's lit tiles in PAIRS (sys.pair_info): per pair ONE wait for everything fetched a pair ago, the
    // layer rows out of the wave's LDS image into registers, the block's shared data of both tiles into its slots,
    // ONE barrier, then the fetches of the next pair (in flight during the two tiles of this one) and the tiles.
    const std::integral_constant<int, 1> dm;
    const int np = sys.pair_count[r];
    const const_int_p pinfo = (const_int_p)(unsigned long long)(sys.pair_info + r * (2 * ((ntl + 1) / 2 + 2)));
    // loader role of the lane: row rr of an 8-row block, chunk (lane & 7) ^ rr of the 128-byte row piece
    const int rr = lane >> 3, kk = (lane & 7) ^ rr;
    unsigned dvo[NL][2];
#pragma unroll
    for (int l = 0; l < NL; l++) {
      const DevLayer &L = sys.layers[l];
      int py = L.toy + st.origin[(e * sys.nlayers + l) * 2 + 1]; py -= (py >= L.dim) ? L.dim : 0;
#pragma unroll
      for (int b = 0; b < 2; b++) {
        unsigned pr = (unsigned)(16 * r + 8 * b + rr) + (unsigned)py; pr = min(pr, pr - ldim[l]);
        dvo[l][b] = 4u * (pr * (ldim[l] + RING_PAD)) + 16u * (unsigned)kk;
      }
    }
    // reader role: row c = 8 bc + rc, chunk 4 h + q of tile h
    const int bc = c >> 3, rc = c & 7;
    const char *rdp[2];
#pragma unroll
    for (int h = 0; h < 2; h++) rdp[h] = dimg + bc * FWD_BLK + 16 * (rc * 8 + ((4 * h + q) ^ rc));
    const unsigned dimg_lds = (unsigned)(unsigned long long)dimg;       // LDS byte address of the wave's images
    FrameRaw<NL, OTF> A, B;
    unsigned mrA, mrB;
    float fA, fB;
    const unsigned shb_lds = (unsigned)(unsigned long long)shb + 1024u * (unsigned)wv;   // this wave's quarter of a slot
    auto dma16 = [&](unsigned vo, __amdgpu_buffer_rsrc_t rs, unsigned lds_addr, unsigned so) {
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(vo), "s"(rs), "s"(lds_addr), "s"(so) : "memory");
    };
    // the block's shared data of a pair, one quarter per wave, filled in place (par: parity of the pair, the slots
    // are double-buffered)
    auto issue_shared = [&](int ia, int ib, int par) {
      const int ta = (ia >> 24) & 0x7F, tb = (ib >> 24) & 0x7F;
      dma16(shvo, shrs, shb_lds + (unsigned)par * 8192u, (unsigned)ta << shstep);
      dma16(shvo, shrs, shb_lds + (unsigned)par * 8192u + 4096u, (unsigned)tb << shstep);
    };
    auto issue = [&](int ia, int ib) {
      const int ta = (ia >> 24) & 0x7F, tb = (ib >> 24) & 0x7F;
      mrA = *reinterpret_cast<const uint16_t *>(mkb + 2u * (unsigned)ta + mvo);
      mrB = *reinterpret_cast<const uint16_t *>(mkb + 2u * (unsigned)tb + mvo);
      fA = cflux[ia & 0xFFFF];
      fB = cflux[ib & 0xFFFF];
#pragma unroll
      for (int l = 0; l < NL; l++) {
        unsigned sx = 16u * (unsigned)(ta & ~1) + lpxs[l]; sx -= (sx >= ldim[l]) ? ldim[l] : 0u;   // scalar; 32 pixels never wrap
        const unsigned so = 4u * sx;
#pragma unroll
        for (int b = 0; b < 2; b++) dma16(dvo[l][b], lrs[l], dimg_lds + l * FWD_IMG + b * FWD_BLK, so);
      }
    };
    int ia = pinfo[0], ib = pinfo[1];
    if (np > 0) { issue_shared(ia, ib, 0); issue(ia, ib); }
    // head of a pair: its data out of the wave's image, the barrier, the fetches of the next pair; returns its slots
    auto head = [&](int k, int ja, int jb) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this pair's layer images, shared quarters and masks have landed
#pragma unroll
      for (int l = 0; l < NL; l++) {
        const float4 va = *reinterpret_cast<const float4 *>(rdp[0] + l * FWD_IMG);
        const float4 vb = *reinterpret_cast<const float4 *>(rdp[1] + l * FWD_IMG);
        A.L[l][0] = va.x; A.L[l][1] = va.y; A.L[l][2] = va.z; A.L[l][3] = va.w;
        B.L[l][0] = vb.x; B.L[l][1] = vb.y; B.L[l][2] = vb.z; B.L[l][3] = vb.w;
      }
      A.mrow = mrA; A.F = fA; B.mrow = mrB; B.F = fB;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the image has been read: the next pair may overwrite it
      float4 *slots = shb + (k & 1) * 512;
      __syncthreads();
      if (k + 1 < np) { issue_shared(ja, jb, (k + 1) & 1); issue(ja, jb); }
      return slots;
    };
    // two fully lit sub-aperture tiles: the pair block (slopes-only fp32)
    auto both_full = [&](int ia, int ib) {
      constexpr int FW_PAIR = FW_LIT | FW_FULL | FW_SUB;
      return QF && (ia & ib & FW_PAIR) == FW_PAIR && !dbg;
    };
    // Runs of such pairs -- the inside of a stripe -- are a loop of their own, one basic block: in one loop with the
    // tile() path behind a branch the allocator kept the stripe's accumulators in other registers on the two sides
    // and copied them back at the end of every pair (seventeen v_mov).
    int k = 0;
    while (k < np) {
      if (both_full(ia, ib)) {
        do {
          const int ja = pinfo[2 * k + 2], jb = pinfo[2 * k + 3];
          const float4 *slots = head(k, ja, jb);
          if constexpr (QF) pair_block(ia, ib, A, B, slots);
          ia = ja; ib = jb; k++;
        } while (k < np && both_full(ia, ib));
      } else {
        const int ja = pinfo[2 * k + 2], jb = pinfo[2 * k + 3];
        float4 *slots = head(k, ja, jb);
        if (ia & FW_LIT) tile(ia, 0, A, A, dm, slots);
        if (ib & FW_LIT) tile(ib, 0, B, B, dm, slots + 256);
        ia = ja; ib = jb; k++;
      }
    }
  } else {
  // The stripe's lit tiles, compact (sys.lit_info[r][k], tile index in bits 24..30; the entries past the last one
  // repeat it, so the prefetches at the end of the list need no test: the last tile is loaded again, from L2, and
  // dropped).  D = 2 tiles of loads are in flight (as many register sets, the list walked in groups of that
  // many; the tiles left over come last, on data the last group prefetched).  The list is read with scalar loads.
  const std::integral_constant<int, 0> nd;
  const std::integral_constant<int, 2> nf;
  const int nl = sys.lit_count[r];
  const const_int_p linfo = (const_int_p)(unsigned long long)(sys.lit_info + r * (ntl + 8));
  {
    constexpr int D = 2;
    FrameRaw<NL, OTF> raw[D];
    int inf[D];
#pragma unroll
    for (int d = 0; d < D; d++) { inf[d] = linfo[d]; fetch(inf[d], raw[d]); }
    const int rem = nl % D, nfull = nl - rem;
    for (int k = 0; k < nfull; k += D) {
      int nx[D];
#pragma unroll
      for (int d = 0; d < D; d++) nx[d] = linfo[k + D + d];
#pragma unroll
      for (int d = 0; d < D; d++) tile(inf[d], nx[d], raw[d], raw[d], nd, nullptr);
#pragma unroll
      for (int d = 0; d < D; d++) inf[d] = nx[d];
    }
#pragma unroll
    for (int d = 0; d + 1 < D; d++)
      if (rem > d) tile(inf[d], inf[d], raw[d], raw[d], nf, nullptr);
  }
  }
  if (!active) return;
  if constexpr (QF) {
    // ---- slopes of the stripe's sub-apertures: lane t = tile t (the moments were written by this wave: its LDS
    // accesses complete in order)
    if (do_cog && !(dbg & 1)) {
      for (int tt = lane; tt < ntl; tt += 64) {
        const int ti = sys.tile_info[r * ntl + tt];
        if (ti & FW_SUB) {
          const float4 m = qmom[tt];
          float sx, sy;
          qf_slopes(sys, m.x, m.z, m.y, sx, sy);
          float *sl = st.slopes + (long long)e * sys.nslope;
          sl[ti & 0xFFFF] = sx;
          sl[sys.nvalid + (ti & 0xFFFF)] = sy;
        }
      }
    }
  }
  // ---- PSF rows of this stripe.  Register j of lane (q, c): row y = 4q + j, column c of the merged operand
  // (c < 8: cos of k = c + 1; c >= 8: sin of k = c - 7); the other half of a +-k pair sits in lane c ^ 8 of
  // the same 16-lane row (row_ror:8).  Lanes c < 8 write kx = -(c + 1), lanes 8 .. 14 kx = +(c - 7), lane 15
  // (k = 8 has no +8 in the window [-8, 8)) writes kx = 0 from the row sums.
  if constexpr (PK) {
    R0r += R0rp.x + R0rp.y; R0i += R0ip.x + R0ip.y;
    sd += sdp.x + sdp.y; sd2 += sd2p.x + sd2p.y; sm += 4.f * (float)nfull;
  }
  R0r += __shfl_xor(R0r, 16); R0r += __shfl_xor(R0r, 32);          // -> every lane: full sum of row y = c
  R0i += __shfl_xor(R0i, 16); R0i += __shfl_xor(R0i, 32);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float oa = dpp_f<0x128>(PA[j]), ob = dpp_f<0x128>(PB[j]);
    const float z0r = __shfl(R0r, 4 * q + j), z0i = __shfl(R0i, 4 * q + j);
    float rr, ri;
    int kxi;
    if (c < 8) { rr = PA[j] - ob; ri = PB[j] + oa; kxi = 7 - c; }
    else if (c < 15) { rr = oa + PB[j]; ri = ob - PA[j]; kxi = c + 1; }
    else { rr = z0r; ri = z0i; kxi = 8; }
    float2 *o = reinterpret_cast<float2 *>(TR) + ((long long)el * pd + (16 * r + 4 * q + j)) * 16 + kxi;
    *o = make_float2(rr, ri);
  }
  sd = wave_sum(sd); sd2 = wave_sum(sd2); sm = wave_sum(sm);
  if (lane == 0) {
    float *pp = TPART + ((long long)el * nblk + r) * 4;
    pp[0] = sd; pp[1] = sd2; pp[2] = sm; pp[3] = 0.f;
  }
}

int launch_frame_wave(const FrameLaunch &a, int variant[6]) {
  const bool otf = a.otf, noise = a.noise, cube = a.cube, hp = a.hp;
  const int nb = a.nb;
// the events ride on the dispatch itself (its start / completion signal): no marker packets of their own
// on the queue in front of and behind the kernel
#define FW(NL, NB, OTF, NZ, WC, HP)                                                                                   \
  do {                                                                                                                \
    hipExtLaunchKernelGGL((k_frame_wave<NL, NB, OTF, NZ, WC, HP>), a.grid, dim3(256), a.lds, a.stream, a.ev_start,    \
                          a.ev_done, 0, *a.sys, a.ds, a.b, a.n, a.cog, a.TR, a.TP, a.nblk);                           \
    variant[0] = NL; variant[1] = NB; variant[2] = OTF; variant[3] = NZ; variant[4] = WC; variant[5] = HP;            \
  } while (0)
#define FW_H(NL, NB, OTF, NZ, WC) do { if (hp) FW(NL, NB, OTF, NZ, WC, true); else FW(NL, NB, OTF, NZ, WC, false); } while (0)
#define FW_NC(NL, NB, OTF)                                                                     \
  do {                                                                                          \
    if (noise) { if (cube) FW_H(NL, NB, OTF, true, true); else FW_H(NL, NB, OTF, true, false); }     \
    else { if (cube) FW_H(NL, NB, OTF, false, true); else FW_H(NL, NB, OTF, false, false); }         \
  } while (0)
#define FW_L(NL)                                                          \
  do {                                                                    \
    if (!otf) FW_NC(NL, 1, false);                                        \
    else if (nb == 1) FW_NC(NL, 1, true);                                 \
    else FW_NC(NL, 2, true);                                              \
  } while (0)
  if (a.nl == 1) FW_L(1); else FW_L(3);
#undef FW_L
#undef FW_NC
#undef FW_H
#undef FW
  LAUNCHCHK();
  return 0;
}
