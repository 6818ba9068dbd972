// aomarl_env_host.h -- the environment's context as the translation units that trace on it see it: aomarl_capi_dmreg.hip,
// aomarl_lgs.hip, aomarl_tomo.hip, aomarl_field.hip, aomarl_mcao.hip.  struct aomarl_ctx stays private to aomarl_capi.hip,
// which defines everything declared in the first part; these units hold a context by pointer only.  The second part is what
// the field and the altitude mirrors ask of each other.  Not part of the C ABI: hidden visibility.
#pragma once
#include "aomarl_host.h"

#include <string.h>
#include <string>
#include <vector>

// what a unit reads of a context, taken once per call
struct EnvView {
  DevSys sys;                      // the static description with the layer windows moved by the wind accumulators' remainder ("subpixel_flow"): what a trace kernel takes
  int nlayers, ndm;
  float delay;
  const float *frac_x, *frac_y;    // [nlayers] that remainder with "subpixel_flow", else null
};
AOMARL_LOCAL EnvView env_view(const aomarl_ctx *c);
AOMARL_LOCAL DevState dev_state(const aomarl_state *st);

// frames or screens that run ahead of the chains: ENV_PIPELINED a pipelined frame (aomarl_set_frame_pipeline),
// ENV_RESET_PREFETCHED the next episode's screens (aomarl_reset_prefetch_begin).  env_refuse_busy: 0, or the refusal of
// the first of the two in that order, "<who>: ..." -- the one place that words it
enum { ENV_PIPELINED = 1, ENV_RESET_PREFETCHED = 2 };
AOMARL_LOCAL int env_busy(const aomarl_ctx *c);
AOMARL_LOCAL int env_refuse_busy(const char *who, const aomarl_ctx *c);
// what a trace of environments [b, b + n) waits for, in this order: the range and the state's buffers (check_range), a
// prefetched move of the atmosphere, and -- AOMARL_TRACE_DMS in flags while the stack-array shapes exist only as
// voltages ("defer_dm_shape") -- those shapes
AOMARL_LOCAL int env_trace_ready(aomarl_ctx *c, aomarl_state *st, int b, int n, int flags, void *stream);

// a kernel of the environment on a unit's own buffer (a kernel is launched from the unit that defines it): k_inc_u32 on
// p[0 .. n)
AOMARL_LOCAL int launch_inc_u32(uint32_t *p, int n, hipStream_t s);

// ---- the science field (aomarl_field.hip) as aomarl_field_attach_mirrors / _detach_mirrors (aomarl_mcao.hip) see it.
// base: planes, nmirrors, stride and dim of the attached object (FieldMirArgs, aomarl_field_host.h); off: the
// directions' offsets on its planes, HOST [ndir][nmirrors][2]
struct FieldMirArgs;
AOMARL_LOCAL void field_dims(const aomarl_field *f, int *nenv, int *ndir, int *pupdiam);
AOMARL_LOCAL void field_set_mirrors(aomarl_field *f, const aomarl_mcao *owner, const FieldMirArgs &base, const float *off);
AOMARL_LOCAL void field_clear_mirrors(aomarl_field *f);
