// stage_plan_host_check.cpp -- a stand-alone host program around aomarl_stage_plan_host.h (which instantiation of the
// staged Shack-Hartmann and science-target kernels a call gets, its grid and its dynamic LDS), meant to be built with
// the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o stage_plan_host_check stage_plan_host_check.cpp
// No GPU, no HIP.  It walks the whole query space of both planners -- every combination of the booleans, nlayers 1 | 3,
// hw 4 | 8 | 16, npsf 64 | 4096 | 4098, nvalid 1 | 5 | 1264, n 1 | 7 | 4096, pupdiam 48 | 320 with the work layout's
// stripe count -- and requires of every plan what a launch needs: a grid inside its bounds, LDS that the kernel's carve-up
// fits and a workgroup may ask for, stripes that cover the pupil.  Exit status 0: all held, and the line
// "stage_plan_host_check: ok (<spot queries> + <target queries> queries)".
//     stage_plan_host_check --table     also prints one line per query: the facts, then the refusal's text or the
//                                       instantiation, its arguments, grid and LDS (tests/test_stage_plan.py compares
//                                       each with what the entry points decided before there was a plan)
#include "aomarl_stage_plan_host.h"
#include <stdio.h>
#include <string.h>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static const char *tf(bool b) { return b ? "true" : "false"; }

int main(int argc, char **argv) {
  const bool table = argc >= 2 && !strcmp(argv[1], "--table");
  const int kLayers[2] = {1, 3}, kValid[3] = {1, 5, 1264}, kEnv[3] = {1, 7, 4096};
  const int kHw[3] = {4, 8, 16}, kNpsf[3] = {64, 4096, 4098}, kPd[2] = {48, 320};
  unsigned long long nspot = 0, ntarget = 0, seen_refusal[5] = {0, 0, 0, 0, 0}, seen_family[2] = {0, 0}, seen_rows[3] = {0, 0, 0};

  // ---- the Shack-Hartmann image
  for (unsigned b = 0; b < (1u << 11); b++)
    for (int nl : kLayers)
      for (int nvalid : kValid)
        for (int n : kEnv) {
#define bit(k) (((b >> (k)) & 1u) != 0)
          SpotQuery q;
          q.from_buf = bit(0); q.noise = bit(1); q.cube = bit(2); q.cog = bit(3); q.no_atmos = bit(4); q.no_dms = bit(5);
          q.force_generic_spot = bit(6); q.production_layout = bit(7);
          q.has_wfs_phase = bit(8); q.has_bincube = bit(9); q.wfs_all_int = bit(10);
          q.nlayers = nl; q.nvalid = nvalid; q.n = n;
#undef bit
          const SpotPlan p = plan_spot(q);
          nspot++; seen_refusal[p.refusal]++;
          if (table)
            printf("spot from_buf=%d noise=%d cube=%d cog=%d no_atmos=%d no_dms=%d force_generic_spot=%d production_layout=%d "
                   "wfs_phase=%d bincube=%d wfs_all_int=%d nlayers=%d nvalid=%d n=%d -> ",
                   q.from_buf, q.noise, q.cube, q.cog, q.no_atmos, q.no_dms, q.force_generic_spot, q.production_layout,
                   q.has_wfs_phase, q.has_bincube, q.wfs_all_int, nl, nvalid, n);
          if (p.refusal != SPOT_OK) {
            REQUIRE(spot_refusal_text(p.refusal)[0] != 0);
            if (table) printf("refused: %s\n", spot_refusal_text(p.refusal));
            continue;
          }
          seen_family[p.family]++;
          // every wave of the grid has a sub-aperture to start on, or the grid is the one block that must exist
          REQUIRE(p.gx >= 1 && (p.gx - 1) * SPOT_WAVES < nvalid && p.gy == n && p.block == SPOT_WAVES * 64);
          REQUIRE((long long)p.gx * SPOT_WAVES * n < SPOT_WAVES_WANTED + SPOT_WAVES * (long long)n || p.gx == 1);
          REQUIRE(p.cube || p.cog);                                      // something is produced
          if (p.family == SPOT_FAST) REQUIRE((p.nl == 1 || p.nl == 3) && !q.from_buf && !q.no_atmos && !q.no_dms);
          if (p.family == SPOT_GENERIC) REQUIRE(p.from_buf == q.from_buf && p.nl == 0);
          if (p.cube) REQUIRE(q.has_bincube);
          if (p.family == SPOT_GENERIC && p.from_buf) REQUIRE(q.has_wfs_phase);
          if (!(p.family == SPOT_GENERIC && p.from_buf)) REQUIRE(q.wfs_all_int);
          if (table) {
            if (p.family == SPOT_FAST) printf("k_wfs_spot_fast<%d, %s, %s>(cog=%d)", p.nl, tf(p.noise), tf(p.cube), p.cog);
            else printf("k_wfs_spot<%s, %s, %s>(no_atmos=%d, no_dms=%d, cog=%d)", tf(p.from_buf), tf(p.noise), tf(p.cube), p.no_atmos, p.no_dms, p.cog);
            printf(" grid=%dx%d block=%d\n", p.gx, p.gy, p.block);
          }
        }
  for (int k = 0; k < 5; k++) REQUIRE(seen_refusal[k] > 0);
  REQUIRE(seen_family[SPOT_GENERIC] > 0 && seen_family[SPOT_FAST] > 0);

  // ---- the science target's PSF
  for (unsigned b = 0; b < (1u << 4); b++)
    for (int hw : kHw)
      for (int npsf : kNpsf)
        for (int pd : kPd)
          for (int nl : kLayers)
            for (int n : kEnv) {
              TargetQuery q;
              q.from_buf = b & 1u; q.production_layout = b & 2u; q.force_valu_target = b & 4u; q.force_generic_target = b & 8u;
              q.hw = hw; q.npsf = npsf; q.pupdiam = pd; q.nlayers = nl; q.n = n;
              const int RB = STAGE_BLOCK / (2 * hw);                       // the work layout's stripe: rows of a block
              q.nblk = (pd + RB - 1) / RB;
              const TargetPlan p = plan_target(q);
              ntarget++; seen_rows[p.rows]++;
              // the rows kernel's carve-up of its dynamic LDS, region by region as the kernel lays them out
              const size_t planes = p.rows == ROWS_FAST ? 2 * (size_t)(2 * TGT_TILE) : p.rows == ROWS_MFMA ? 2 * (size_t)TGT_TILE
                                                                                                        : 2 * (size_t)(RB * TGT_XC);
              const size_t red = p.rows == ROWS_VALU ? TGT_RED_VALU : TGT_RED_MFMA;
              const size_t tw = npsf <= TGT_TW_MAX ? 2 * (size_t)npsf : 0;
              REQUIRE(p.rows_lds == sizeof(float) * (planes + red + tw));
              REQUIRE(p.rows_lds <= 64 * 1024);                            // what a workgroup may ask for without opting in
              REQUIRE(red >= 3 * (size_t)STAGE_BLOCK);                     // every rows kernel ends with three sums over the block
              // matrix-core kernels: 16 rows, 16 frequencies; the stripes cover the pupil
              if (p.rows != ROWS_VALU) REQUIRE(hw == 8 && !q.force_valu_target && RB == 16 && p.finish == FINISH_MFMA);
              if (p.rows == ROWS_VALU) REQUIRE(p.finish == FINISH_VALU && (hw != 8 || q.force_valu_target));
              if (p.rows == ROWS_FAST) REQUIRE(!q.from_buf && q.production_layout && !q.force_generic_target && (p.nl == 1 || p.nl == 3));
              if (p.rows != ROWS_FAST) REQUIRE(p.from_buf == q.from_buf && p.nl == 0);
              REQUIRE(p.rows_gx == q.nblk && p.rows_gx * RB >= pd && p.rows_gy == n && p.finish_gx == n && p.nblk == q.nblk);
              REQUIRE(p.block == STAGE_BLOCK);
              if (table) {
                printf("target hw=%d npsf=%d pupdiam=%d nlayers=%d from_buf=%d production_layout=%d force_valu_target=%d "
                       "force_generic_target=%d nblk=%d n=%d -> ",
                       hw, npsf, pd, nl, q.from_buf, q.production_layout, q.force_valu_target, q.force_generic_target, q.nblk, n);
                if (p.rows == ROWS_FAST) printf("k_target_rows_fast<%d>", p.nl);
                else printf("%s<%s>", p.rows == ROWS_MFMA ? "k_target_rows_mfma" : "k_target_rows", tf(p.from_buf));
                printf(" grid=%dx%d block=%d lds=%zu nblk=%d | %s grid=%d block=%d\n", p.rows_gx, p.rows_gy, p.block, p.rows_lds, p.nblk,
                       p.finish == FINISH_MFMA ? "k_target_finish_mfma" : "k_target_finish", p.finish_gx, p.block);
              }
            }
  for (int k = 0; k < 3; k++) REQUIRE(seen_rows[k] > 0);
  printf("stage_plan_host_check: ok (%llu + %llu queries)\n", nspot, ntarget);
  return 0;
}
