// aomarl_frame_host.h -- the one-pass frame kernel (aomarl_frame.hip) as the environment launches it
// (frame_fused_impl, aomarl_capi_composites.hip): which instantiation, and what one launch of it takes.
#pragma once
#include "aomarl_host.h"

struct FrameLaunch {
  int nl, nb;                          // k_frame_wave<NL, NB, OTF, NOISE, WRITE_CUBE, HP>: layers 1 or 3; lattice blocks 1 or 2
  bool otf, noise, cube, hp;
  dim3 grid;
  size_t lds;                          // dynamic LDS bytes of a workgroup (frame_lds(...).total, plus any padding)
  hipStream_t stream;
  hipEvent_t ev_start, ev_done;        // ride on the dispatch itself; nullptr: none
  const DevSys *sys;
  DevState ds;
  int b, n, cog;
  float *TR, *TP;
  int nblk;
};
// one launch; variant = the template arguments of the instantiation it launched
AOMARL_LOCAL int launch_frame_wave(const FrameLaunch &a, int variant[6]);
