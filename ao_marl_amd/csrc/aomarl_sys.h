// aomarl_sys.h -- the system description the kernels take as an argument (DevSys and its layers and mirrors) and the ring
// layout's constant: plain structs, no HIP include, so the host-only plan that fills them (aomarl_create_plan_host.h)
// and its stand-alone check compile without HIP.  aomarl_dev.h includes this; the layout is part of every kernel's
// argument block.
#pragma once
#include <stdint.h>

#include "../../include/aomarl.h"

struct DevLayer {
  int dim, ns;
  long long screen_off;          // floats from the env's screen base
  const uint32_t *istx, *isty;   // packed (x | y << 16) logical stencil coordinates
  const uint32_t *istT;          // istx with x and y exchanged: the x stencil of the TRANSPOSED screen (reset)
  const float *AB;               // [dim][ldab]: row r = [A[r][0..ns) | B[r][0..dim)]
  int ldab;
  const float *ABt;              // [ns + dim][ldt], ldt = dim rounded up to 64 (zero padded): the transpose, small screens only
  int ldt;
  float amp;
  float wxo, wyo, txo, tyo;      // float offsets
  int wox, woy, tox, toy;        // integer parts
};

struct DevDm {
  int type, dim, nact, ss;
  long long shape_off;           // floats from the env's dm_shape base
  int com_off;                   // first command index
  const float *influ;
  const int32_t *influpos, *ninflu, *influstart;
  float wxo, wyo, txo, tyo;
  int wox, woy, tox, toy;
  // stack-array fast path: every actuator shares one separable patch influ[a][b] = prof[a] prof[b]
  // and sits on a regular lattice (i1min + pitch*gx, j1min + pitch*gy); grid[gy*gw+gx] = actuator
  // index or -1.  0 = use the generic gather tables.
  int sep, pitch, i1min, j1min, gw, gh;
  const int32_t *grid;
  const float *prof;
};

struct DevSys {
  int n, pupdiam;
  const float *mpupil, *spupil;
  int nvalid, pdiam, nfft, npix, nrebin, nxsub;
  const int32_t *phasemap;
  const int32_t *sub_xy;         // [nvalid] packed (x0 | y0 << 16): top-left phase pixel
  const float *halfxy;
  const int32_t *binmap;
  const float *flux;
  const int32_t *validx, *validy;
  float nphot, wfs_inv_lambda, noise, cog_offset, cog_scale, subapd;
  int nlayers;
  DevLayer layers[AOMARL_MAX_LAYERS];
  int ndm;
  DevDm dms[AOMARL_MAX_DMS];
  float tar_inv_lambda;
  int npsf, hw;
  const float *psf_tw;           // [npsf][2] cos, sin of 2 pi j / npsf
  float ref_peak;
  int nactu, nslope;
  int wfs_all_int, tar_all_int;  // every offset of that path is an integer
  long long screen_stride, shape_stride;
  // ---- fused frame kernel (WFS + science path share every phase pixel: the 16x16 sub-aperture
  // tiles ARE the tiles of the pupil grid): available when the geometry lines up (see create)
  int fused_ok, ntiles;          // ntiles = pupdiam / 16 tiles per axis
  const int32_t *stripe_order;   // [ntiles] stripes by decreasing number of lit tiles
  const int32_t *tile_info;      // [ntiles][ntiles] (stripe, tile): sub-aperture | lit / full / has-sub bits
  const int32_t *lit_info;       // [ntiles][ntiles + 8]: the stripe's LIT tiles in x order, compact: tile_info | tile << 24;
                                 //   entries past the last one repeat it
  const int32_t *lit_count;      // [ntiles] lit tiles per stripe
  // the same walk in PAIRS of adjacent tiles (2 g, 2 g + 1) with at least one lit tile: [ntiles][(ntiles + 1) / 2 + 2][2]
  // entries (tile A, tile B) of the lit_info form (bit 16 clear: that tile of the pair is not lit; the tile index is
  // valid either way); entries past the last pair repeat it
  const int32_t *pair_info;
  const int32_t *pair_count;     // [ntiles] pairs per stripe
  const uint16_t *tile_mask;     // [pupdiam][ntiles]: bit b = spupil[y][16 t + b] != 0
  // stack-array DM phase from the command lattice inside the frame kernel (separable lattice whose
  // pitch divides the tile size): nodes per axis that reach a tile <= 4 otf_nb
  int otf_ok, otf_nb, otf_tpn;   // otf_tpn = lattice nodes per tile step (16 / pitch)
  int otf_gx0, otf_gy0;          // first node column / row that reaches tile 0 / stripe 0
  int otf_xoff, otf_yoff;        // DM pixel of the tile origin minus the position of that node
  int otf_latw;                  // lattice columns a stripe can touch
  // PSF operand of the frame kernel for lane (q, c) of tile t, 16 B each: column c of [cos k X (k = 1..8) |
  // sin k X (k = 1..8)], X = 16 t + 4 q + j, j = 0..3
  const void *psf_tw_h;          // [ntiles][64] x 8 halfs: [hi(j = 0..3) | lo(j = 0..3)]  (split-fp16 form)
  const void *psf_tw_f;          // [ntiles][64] x 4 floats                                  (fp32 form)
  const float *qf_tab;           // [64 lanes][8]: SpotQf of each lane (built on the host at create: aomarl_qf4_host.h)
  // tip-tilt planes in pupil coordinates, 4 pixels of a row at a time: [pupdiam][pupdiam / 4] x [x0 x1 x2 x3 | y0 y1 y2 y3]
  const float *tt_pk;
};

// Ring-buffered screen: physical rows are n + RING_PAD floats long, columns [n, n + RING_PAD) mirror columns
// [0, RING_PAD) (ring_idx in aomarl_dev.h).
// (56, not 32: with the screens of the production files -- 648 and 168 pixels -- the row pitch is then a multiple of
// 128 bytes, every row of a tile starts at the same offset inside its line; see k_reset_env)
#define RING_PAD 56
static_assert(RING_PAD >= 32 && RING_PAD % 4 == 0, "the frame kernel's pair fetch reads 32 consecutive pixels in 16-byte pieces");
