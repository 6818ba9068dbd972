// aomarl_stage_host.h -- the staged sensor kernels (aomarl_wfs.hip) and the science target's kernels (aomarl_target.hip)
// as the environment launches them: a plan of aomarl_stage_plan_host.h in, one launch out.  No other unit names one of
// these kernels.  Not part of the C ABI: hidden visibility.
#pragma once
#include "aomarl_host.h"
#include "aomarl_stage_plan_host.h"

// ---- aomarl_wfs.hip
// k_wfs_spot<FROM_BUF, NOISE, WRITE_CUBE> or k_wfs_spot_fast<NL, NOISE, WRITE_CUBE>, as the plan says (not a refused one)
AOMARL_LOCAL int launch_spot(const SpotPlan &p, const DevSys &sys, const DevState &st, int env_begin, hipStream_t s);
// k_cog / k_slopes_geom: one wave per sub-aperture of the n environments from env_begin
AOMARL_LOCAL int launch_cog(const DevSys &sys, const DevState &st, int env_begin, int n, hipStream_t s);
AOMARL_LOCAL int launch_slopes_geom(const DevSys &sys, const DevState &st, int env_begin, int n, hipStream_t s);

// ---- aomarl_target.hip
// the plan's rows kernel: first DFT axis into TR, the variance partials into TP
AOMARL_LOCAL int launch_target_rows(const TargetPlan &p, const DevSys &sys, const DevState &st, int env_begin, float *TR,
                                    float *TP, hipStream_t s);
// The finish (second axis, |G|^2, the peak fit, the variance) of n environments into PEND.  FINISH_MFMA also counts the
// frame in frame[0 .. n) when that is not null (the one-pass path).  ev: events that ride on the dispatch itself -- each
// may be null; without an `ev` the launch is a plain one.
struct FinishEvents { hipEvent_t start, done; };
AOMARL_LOCAL int launch_target_finish(TargetFinish kind, const DevSys &sys, const float *TR, const float *TP, int nblk,
                                      float *PEND, uint32_t *frame, int n, hipStream_t s, const FinishEvents *ev = nullptr);
// k_strehl_commit: publish the pending windows PEND of the n environments from env_begin
AOMARL_LOCAL int launch_strehl_commit(const DevSys &sys, const DevState &st, int env_begin, int n, const float *PEND,
                                      hipStream_t s);
// k_strehl_reset / k_strehl_fit_le on the n records and long-exposure sums from env_begin of st (the science field
// launches them on its own buffers)
AOMARL_LOCAL int launch_strehl_reset(const DevSys &sys, const DevState &st, int env_begin, int n, hipStream_t s);
AOMARL_LOCAL int launch_strehl_fit_le(const DevSys &sys, const DevState &st, int env_begin, int n, hipStream_t s);
