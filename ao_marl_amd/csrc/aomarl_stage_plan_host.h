// aomarl_stage_plan_host.h -- what the two staged stages of the environment decide before they launch anything: the
// Shack-Hartmann image (aomarl_comp_image -> aomarl_wfs.hip) and the science target's PSF (aomarl_target_psf ->
// aomarl_target.hip).  No HIP include and no global: the facts come in as plain structs (the two entry points in
// aomarl_capi_stages.hip are the one place that reads them off the context, the state and the call's flags), so the
// stand-alone host program (stage_plan_host_check.cpp) walks the same text over every combination of them, also under
// the address and undefined-behaviour sanitizers; tests/test_stage_plan.py compares every plan with the conditions and
// formulas the entry points spelled out before there was a plan.  The launchers (aomarl_stage_host.h) take a plan and
// turn it into one instantiation: the only place a template argument of these kernels is named.
//
// The rules:
//
//   spot    refused, in this order: FROM_PHASE_BUFFER without st->wfs_phase; the fused raytrace without integer layer
//           offsets; WRITE_BINCUBE without st->bincube; neither bincube nor slopes asked for.
//           SPOT_FAST   = !from_buf && !no_atmos && !no_dms && !"force_generic_spot" && production layout:
//                         k_wfs_spot_fast<NL = 1 | 3, NOISE, WRITE_CUBE>
//           SPOT_GENERIC  otherwise: k_wfs_spot<FROM_BUF, NOISE, WRITE_CUBE>
//           grid    persistent waves, enough blocks per environment to fill the chip about twice (256 CUs x 32 waves
//                   x 2 = SPOT_WAVES_WANTED): gx = clamp(ceil(SPOT_WAVES_WANTED / (SPOT_WAVES n)), 1,
//                   ceil(nvalid / SPOT_WAVES)) by n, blocks of SPOT_WAVES waves
//   target  ROWS_FAST   = hw == 8 && !"force_valu_target" && !"force_generic_target" && !from_buf && production layout:
//                         k_target_rows_fast<NL = 1 | 3>, two tiles (double buffer) per plane
//           ROWS_MFMA   = hw == 8 && !"force_valu_target", not that: k_target_rows_mfma<FROM_BUF>, one tile per plane
//           ROWS_VALU     otherwise: k_target_rows<FROM_BUF>, 256 / (2 hw) rows of TGT_XC columns per plane
//           finish  FINISH_MFMA behind the two matrix-core row kernels, FINISH_VALU behind ROWS_VALU
//           LDS     of the rows kernel: the real and the imaginary plane, the reduction scratch, and the npsf twiddles
//                   (float2) when npsf <= TGT_TW_MAX
//           grids   rows: nblk by n (nblk: the work layout's stripes of 256 / (2 hw) pupil rows); finish: n
#pragma once
#include <stddef.h>

// ---- what the launch arithmetic shares with the kernels: one definition for both
// k_wfs_spot / k_wfs_spot_fast: waves (sub-apertures in flight) per block; resident waves the grid aims at
constexpr int SPOT_WAVES = 4, SPOT_WAVES_WANTED = 16384;
// k_target_rows: columns of a staged chunk
constexpr int TGT_XC = 64;
// k_target_rows_mfma / _fast: a 16 x 64 tile of one plane, rows 65 floats apart (bank conflicts)
constexpr int TGT_TILE_PITCH = 65, TGT_TILE = 16 * TGT_TILE_PITCH;
// reduction scratch in floats: [4 waves][2][256] partial tiles (matrix-core kernels), [3][256] sums (k_target_rows)
constexpr int TGT_RED_MFMA = 4 * 2 * 256, TGT_RED_VALU = 3 * 256;
// the PSF twiddles are staged in LDS up to this npsf
constexpr int TGT_TW_MAX = 4096;
constexpr int STAGE_BLOCK = 256;             // threads of every kernel planned here

// ---- the Shack-Hartmann image
struct SpotQuery {
  bool from_buf, noise, cube, cog;           // the call's flags; noise already folded with sys.noise >= 0
  bool no_atmos, no_dms;
  bool force_generic_spot, production_layout;
  int nlayers;
  int nvalid, n;                             // sub-apertures; environments of the call
  bool has_wfs_phase, has_bincube;           // the state's buffers
  bool wfs_all_int;                          // every layer and mirror offset of the WFS direction is a whole pixel
};
enum SpotRefusal { SPOT_OK = 0, SPOT_NEEDS_WFS_PHASE, SPOT_NEEDS_INT_OFFSETS, SPOT_NEEDS_BINCUBE, SPOT_NOTHING_TO_PRODUCE };
static inline const char *spot_refusal_text(SpotRefusal r) {
  switch (r) {
    case SPOT_NEEDS_WFS_PHASE: return "comp_image: FROM_PHASE_BUFFER needs st->wfs_phase";
    case SPOT_NEEDS_INT_OFFSETS: return "comp_image: fused raytrace needs integer layer offsets; use raytrace_wfs + FROM_PHASE_BUFFER";
    case SPOT_NEEDS_BINCUBE: return "comp_image: WRITE_BINCUBE needs st->bincube";
    case SPOT_NOTHING_TO_PRODUCE: return "comp_image: nothing to produce (neither bincube nor slopes)";
    default: return "";
  }
}
enum SpotFamily { SPOT_GENERIC, SPOT_FAST };
struct SpotPlan {
  SpotRefusal refusal;                       // not SPOT_OK: nothing else is set, nothing is launched
  SpotFamily family;
  bool from_buf;                             // SPOT_GENERIC: FROM_BUF
  int nl;                                    // SPOT_FAST: NL
  bool noise, cube;                          // NOISE, WRITE_CUBE
  int no_atmos, no_dms, cog;                 // kernel arguments (SPOT_FAST takes cog alone)
  int gx, gy, block;
};

static inline SpotPlan plan_spot(const SpotQuery &q) {
  SpotPlan p = {};
  p.refusal = q.from_buf && !q.has_wfs_phase ? SPOT_NEEDS_WFS_PHASE
            : !q.from_buf && !q.wfs_all_int ? SPOT_NEEDS_INT_OFFSETS
            : q.cube && !q.has_bincube      ? SPOT_NEEDS_BINCUBE
            : !q.cube && !q.cog             ? SPOT_NOTHING_TO_PRODUCE
                                            : SPOT_OK;
  if (p.refusal != SPOT_OK) return p;
  const bool fast = !q.from_buf && !q.no_atmos && !q.no_dms && !q.force_generic_spot && q.production_layout;
  p.family = fast ? SPOT_FAST : SPOT_GENERIC;
  p.from_buf = !fast && q.from_buf;
  p.nl = fast ? (q.nlayers == 1 ? 1 : 3) : 0;
  p.noise = q.noise; p.cube = q.cube;
  p.no_atmos = q.no_atmos ? 1 : 0; p.no_dms = q.no_dms ? 1 : 0; p.cog = q.cog ? 1 : 0;
  const int want = (SPOT_WAVES_WANTED + SPOT_WAVES * q.n - 1) / (SPOT_WAVES * q.n);
  const int most = (q.nvalid + SPOT_WAVES - 1) / SPOT_WAVES;
  p.gx = want < most ? want : most;
  if (p.gx < 1) p.gx = 1;
  p.gy = q.n;
  p.block = STAGE_BLOCK;
  return p;
}

// ---- the science target's PSF
struct TargetQuery {
  int hw, npsf, pupdiam, nlayers;
  bool from_buf, production_layout, force_valu_target, force_generic_target;
  int nblk, n;                               // the work layout's row stripes; environments of the call
};
enum TargetRows { ROWS_FAST, ROWS_MFMA, ROWS_VALU };
enum TargetFinish { FINISH_MFMA, FINISH_VALU };
struct TargetPlan {
  TargetRows rows;
  int nl;                                    // ROWS_FAST: NL
  bool from_buf;                             // ROWS_MFMA, ROWS_VALU: FROM_BUF
  TargetFinish finish;
  size_t rows_lds;                           // dynamic LDS bytes of a rows workgroup
  int rows_gx, rows_gy, finish_gx, block;
  int nblk;                                  // kernel argument of both stages
};

static inline size_t target_tw_bytes(int npsf) { return npsf <= TGT_TW_MAX ? sizeof(float) * 2 * (size_t)npsf : 0; }

static inline TargetPlan plan_target(const TargetQuery &q) {
  TargetPlan p = {};
  const bool mfma = q.hw == 8 && !q.force_valu_target;
  const bool fast = mfma && !q.force_generic_target && !q.from_buf && q.production_layout;
  p.rows = fast ? ROWS_FAST : mfma ? ROWS_MFMA : ROWS_VALU;
  p.nl = fast ? (q.nlayers == 1 ? 1 : 3) : 0;
  p.from_buf = !fast && q.from_buf;
  p.finish = mfma ? FINISH_MFMA : FINISH_VALU;
  const int RB = STAGE_BLOCK / (2 * q.hw);   // ROWS_VALU: pupil rows of a block
  const size_t floats = fast ? 2 * 2 * TGT_TILE + TGT_RED_MFMA
                      : mfma ? 2 * TGT_TILE + TGT_RED_MFMA
                             : 2 * RB * TGT_XC + TGT_RED_VALU;
  p.rows_lds = sizeof(float) * floats + target_tw_bytes(q.npsf);
  p.rows_gx = q.nblk; p.rows_gy = q.n; p.finish_gx = q.n;
  p.block = STAGE_BLOCK;
  p.nblk = q.nblk;
  return p;
}
