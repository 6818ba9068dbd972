// aomarl_capi.hip -- C ABI (include/aomarl.h) over the gfx950 kernels in aomarl_kernels.hip: context, create / destroy,
// setters and options here; the entry points by concern in aomarl_capi_atmos / _stages / _agents / _step / _extras /
// _composites.hip, included at the end (one translation unit: the environment).  The one-pass frame kernel is a unit of
// its own (aomarl_frame.hip, launched through aomarl_frame_host.h), and so are the staged Shack-Hartmann and science-target
// kernels (aomarl_wfs.hip, aomarl_target.hip, launched through aomarl_stage_host.h with a plan of
// aomarl_stage_plan_host.h).  Mirror registration, the laser guide star, tomography,
// the science field and the altitude mirrors are units of their own; what they may ask of a context is defined at the
// very end (aomarl_env_host.h).
// Host side only sequences kernel launches on the caller's stream; no device<->host copies after
// aomarl_create / aomarl_set_* (aomarl_reset uploads env_count seeds, 4 bytes each).
#include "aomarl_kernels.hip"
#include "aomarl_env_host.h"
#include "aomarl_frame_host.h"
#include "aomarl_stage_host.h"
#include "aomarl_create_plan_host.h"
#include "aomarl_step_plan_host.h"
#include "aomarl_order_host.h"

#include <math.h>
#include <stdlib.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

static thread_local char g_err[512] = "";

int fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return 1;
}


struct aomarl_ctx {
  DevSys sys;
  std::vector<void *> owned;       // device allocations
  // host copies needed for scheduling
  int nlayers = 0, ndm = 0;
  int dim[AOMARL_MAX_LAYERS], ns[AOMARL_MAX_LAYERS], abclass[AOMARL_MAX_LAYERS];
  float deltax[AOMARL_MAX_LAYERS], deltay[AOMARL_MAX_LAYERS];
  int nclass = 0;
  int maxdim = 0, maxK = 0;
  float gain = 0.f, delay = 0.f;
  bool production_layout = false;     // two mirrors, a stack array then a tip-tilt, one or three layers (CreatePlan)
  bool force_generic_dm = false, force_valu_target = false;
  bool force_generic_spot = false, force_generic_target = false, force_unfused_frame = false;
  int dft_mode = -1;                   // frame kernel DFTs: -1 follow the library's precision mode, 0 fp32 MFMAs, 1 split-fp16 ("force_f32_dft")
  bool reset_untransposed = false;     // "reset_untransposed": the reset's x extrusions on the row-major screen itself
  int small_chain = 1;                 // "small_chain": small systems run the control / agent chain of aomarl_env_step as two kernels
  int residual_shortcut = 0;           // "residual_shortcut": aomarl_env_step takes the residual modes from ONE product with v2m . cmat (aomarl_set_slopes2modes)
  int small_move = 1;                  // "small_move": 1 = one k_move_small launch per frame's move where the screens allow it
  bool small_ok = false;               // every layer has dim <= MOVE_SMALL_DIM, ns + dim <= MOVE_SMALL_K (transposed [A|B] uploaded)
  int reset_streams = 2;               // "reset_streams": a batch reset in that many parts side by side, one stream each (1..4)
  bool reset_prefetch_whole = true;    // "reset_prefetch_whole": the prefetched reset as ONE range with the parts' tile and k split
  hipEvent_t ev_reset = nullptr, ev_reset2[3] = {nullptr, nullptr, nullptr};
  bool no_extrude_sg = false;          // "extrude_unfused": scatter and gather of consecutive rounds as separate launches
  bool defer_dm_shape = false;         // composites: stack-array phase from st->voltage on the fly
  int fused_debug = 0;                 // development switches of k_frame_wave (tools/fw_ab.py, tools/fw_pmc.py)
  // "prefetch_atmos": the composite moves the atmosphere of the NEXT frame on a side stream as soon
  // as this frame's image kernels are done, so the extrusion chain runs beside do_control / the
  // agents / next_part_two instead of in front of the next image
  bool prefetch_atmos = false;
  SideOrder order;                 // how the side streams stand against the caller's stream (aomarl_order_host.h)
  // power-of-two scales of the static matrices for the split-f16 GEMM (gemm_scale)
  float cmat_scale = 1.f, v2m_scale = 1.f, m2v_scale = 1.f, s2m_scale = 1.f, ab_scale[AOMARL_MAX_LAYERS] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
  // "subpixel_flow" (experiment, profiles/r03_subpixel_flow.txt): the fractional remainder of the wind
  // accumulators as a sub-pixel shift of the layer windows in the generic bilinear raytrace
  // (aomarl_raytrace_wfs / _target); 0 (default): integer-pixel frozen flow
  bool subpixel_flow = false;
  float frac_x[AOMARL_MAX_LAYERS] = {0, 0, 0, 0, 0, 0, 0, 0}, frac_y[AOMARL_MAX_LAYERS] = {0, 0, 0, 0, 0, 0, 0, 0};
  // "graph_step": aomarl_env_step as a HIP graph (captured once per distinct launch sequence -- extrusion plan,
  // ring position, buffer addresses --, replayed afterwards: one hipGraphLaunch instead of ~25 launches and ~8
  // event operations per step).  capturing: the body is being recorded (no timed / event-carrying dispatch, the
  // side streams fork from and join the caller's stream inside the graph)
  bool graph_step = false, capturing = false;
  hipEvent_t ev_fork = nullptr;
  struct StepGraph { std::vector<long long> key; hipGraphExec_t exec; hipGraph_t graph; unsigned long long arith[AR_N]; int fw_variant[6]; };
  std::vector<StepGraph> graphs;
  unsigned long long graph_hits = 0, graph_captures = 0;
  // bumped by every call that changes a host value captured graphs have baked into their kernel arguments (matrix
  // scales and leading dimensions, nact, gains, per-context options): part of the graph key, together with the
  // process-wide g_cfg_epoch -- a re-uploaded matrix usually lands at the SAME address, so the pointers alone
  // would replay a stale graph
  unsigned long long cfg_epoch = 0;
  const int32_t *sel_checked = nullptr;     // aomarl_env_step: the column selection last validated
  int sel_checked_n = 0, sel_checked_nm = 0;
  int fw_variant[6] = {0, 0, 0, 0, 0, 0};   // template arguments of the last k_frame_wave launch
  char fw_name[96] = {0};
  // "time_frame_kernel": a HIP event pair around every k_frame_wave launch (aomarl_frame_kernel_time)
  bool time_fw = false;
  std::vector<hipEvent_t> fw_ev;            // 2 per timed launch, created on demand
  size_t fw_ev_used = 0;
  std::vector<hipEvent_t> fw_ev_retired;    // timing events a frame in flight still carries as its "done" mark (fw_ev_rewind)
  hipStream_t atm_stream = nullptr, psf_stream = nullptr;
  // (the screens' readers are marked with ev_frame or with the closing event of a timed frame launch: an event
  // record is a barrier packet of its own on the queue, 3-5 us of the step each -- one per frame, not three)
  hipEvent_t ev_frame = nullptr, ev_moved = nullptr, ev_psf = nullptr;
  // frame pipeline (aomarl_set_frame_pipeline): frames on a stream of their own, one step ahead of the chains
  struct FramePipe {
    bool have_twin = false, active = false;
    const float *owner_screens = nullptr;          // the state the twin belongs to
    aomarl_state twin;                             // odd frames: slopes / voltage / dm_shape / work
    int par = 0;                                   // parity (0: st's buffers, 1: the twin's) of the frame in flight
    hipStream_t fstream = nullptr;
    hipEvent_t ev_cmd = nullptr, ev_commit = nullptr, ev_done[2] = {nullptr, nullptr}, ev_psf[2] = {nullptr, nullptr};
    hipEvent_t ev_done_cur[2] = {nullptr, nullptr};  // the event each parity's last frame launch carries (ev_done[], or a timing event)
    bool psf_out[2] = {false, false};              // a PSF finish of that parity may still run
    bool cmd_covers_commit = false;                // ev_cmd was recorded behind the Strehl commit and the PSF-finish wait as well
    bool cmd_covers_psf = false;                   // ev_cmd was recorded behind the PSF-finish wait (not the commit)
    int32_t *snap[2] = {nullptr, nullptr};         // ring origins as of each parity's frame
    size_t snap_ints = 0;
    unsigned long long steps = 0, overlapped = 0, behind = 0;
  } pipe;
  bool pipe_enabled = true;              // "frame_pipeline": 0 = plain call order although a twin is set
  bool pipe_internal = false;            // check_range: the pipelined step itself is calling
  // controller matrices
  float *cmat = nullptr;           // [nactu][ld_s]
  int ld_cmat = 0;
  int nmodes = 0, nact = 0, ld_v2m = 0, ld_m2v = 0;
  float *v2m = nullptr, *m2v = nullptr, *freedom = nullptr;
  float *s2m = nullptr;            // [nmodes][ld_cmat]: v2m . cmat (aomarl_set_slopes2modes)
  int s2m_nmodes = 0;
  int32_t *amodes = nullptr, *amode_inv = nullptr;   // action modes and their inverse map [nmodes]
  float *env_gain = nullptr;       // per-environment integrator gains (aomarl_set_env_gains) or null
  int env_gain_n = 0;
  // per-mode gain factors in Btt coordinates (aomarl_set_modal_gains) or null: device [mgain_rows][mgain_nm], rows = 1
  // (shared) or one per environment; h_mgain: the host copy aomarl_get_modal_gains hands back
  float *mgain = nullptr;
  int mgain_rows = 0, mgain_nm = 0;
  std::vector<float> h_mgain;
  // the on-line optimiser attached to this context (aomarl_modopti_online_attach) or null, and the voltage buffer of the
  // state it was attached with: aomarl_do_control of that state feeds it and its applies write `mgain`
  // mo_mgain_used: the gains the LAST do_control scaled with (device, the size of mgain).  aomarl_rl_control_modes
  // recomposes that frame's command from them: an apply behind frame t must not reach back into frame t's integration.
  // It follows `mgain` one frame late (mo_used_stale: an apply has written mgain since).
  aomarl_modopti_online *mo = nullptr;
  const float *mo_voltage = nullptr;
  float *mo_mgain_used = nullptr;
  bool mo_used_stale = false;
  // the modal predictor attached to this context (aomarl_predictor_attach) or null, and the voltage buffer of the state it
  // was attached with: aomarl_do_control of that state runs it in place of the integration
  aomarl_predictor *pred = nullptr;
  const float *pred_voltage = nullptr;
  uint32_t *seed_stage = nullptr;  // device staging for reset seeds
  int seed_stage_n = 0;
  // aomarl_reset_prefetch_*: the NEXT episode's screens grown in a shadow state while this episode runs
  struct ResetPrefetch *rp = nullptr;
  // aomarl_target_image: DFT tables and per-environment scratch of the full-frame PSF (on demand)
  float *timg = nullptr;
  // geometric controller (aomarl_set_geo): host copies of the lattice tables it is built from,
  // projection operands on the device
  std::vector<int32_t> h_grid;     // [gh][gw] actuator index or -1 (stack-array DM 0)
  std::vector<float> h_prof, h_spupil, h_tt;
  float *geoW = nullptr, *geoUx = nullptr, *geoUy = nullptr, *geoPlanes = nullptr;
  int32_t *geoMap = nullptr;       // stack-array actuator -> j * gh + i of the lattice product
  int geo_ldw = 0, geo_gw = 0, geo_gh = 0, geo_npzt = 0, geo_ldr = 0;
};

static int pipe_drop(aomarl_ctx *c, void *stream);
static void rp_free(aomarl_ctx *c);
// Start the timing events over.  The closing event of a timed frame launch doubles as that frame's "readers are
// done" mark (pipe.ev_done_cur, and what the ledger holds): one that a frame in flight still carries must not be
// re-recorded by a later launch, so it is retired (it stays valid for whoever waits on it) and replaced.
static int fw_ev_rewind(aomarl_ctx *c) {
  void *held[4] = {c->pipe.ev_done_cur[0], c->pipe.ev_done_cur[1], nullptr, nullptr};
  c->order.held_events(held + 2);
  for (size_t i = 0; i < c->fw_ev.size(); i++)
    for (int k = 0; k < 4; k++)
      if (held[k] && c->fw_ev[i] == held[k]) {
        hipEvent_t ne;
        HIPCHK(hipEventCreate(&ne));
        c->fw_ev_retired.push_back(c->fw_ev[i]);
        c->fw_ev[i] = ne;
        break;
      }
  if (c->fw_ev_retired.size() > 64 && !c->pipe.active) {      // nothing in flight refers to them any more
    bool live = false;
    for (hipEvent_t e : c->fw_ev_retired) for (int k = 0; k < 4; k++) live = live || e == held[k];
    if (!live) { for (hipEvent_t e : c->fw_ev_retired) (void)hipEventDestroy(e); c->fw_ev_retired.clear(); }
  }
  c->fw_ev_used = 0;
  return 0;
}
static int frame_fused_impl(aomarl_ctx *c, aomarl_state *st, int b, int n, int flags, void *stream, int slot);
static int next_part_one_sense(aomarl_ctx *c, aomarl_state *st, int b, int n, float *accumx, float *accumy, int image_flags, void *stream);

static unsigned long long g_cfg_epoch = 0;      // process-wide options / precision changes (see aomarl_ctx::cfg_epoch)
const char *aomarl_last_error(void) { return g_err; }
int aomarl_abi_version(void) { return AOMARL_ABI_VERSION; }

int aomarl_set_precision(int mode) {
  g_cfg_epoch++;
  if (mode != AOMARL_PRECISION_F32 && mode != AOMARL_PRECISION_SPLIT_F16) return fail("set_precision: unknown mode %d", mode);
  g_precision = mode;
  g_gemm.split_f16 = mode == AOMARL_PRECISION_SPLIT_F16;
  return 0;
}
int aomarl_get_precision(void) { return g_precision; }
int aomarl_gemm_saturated(unsigned *count, void *stream) {
  if (!count) return fail("gemm_saturated: null argument");
  *count = 0;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !g_gemm_sat[dev]) return 0;       // no split-fp16 GEMM ever ran on this device
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(count, g_gemm_sat[dev], sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (*count) HIPCHK(hipMemsetAsync(g_gemm_sat[dev], 0, sizeof(unsigned), s));
  return 0;
}
int aomarl_arith_families(void) { return AR_N; }
const char *aomarl_arith_family_name(int i) { return (i >= 0 && i < AR_N) ? g_arith_name[i] : ""; }
unsigned long long aomarl_arith_launches(int i) { return (i >= 0 && i < AR_N) ? g_arith[i] : 0ULL; }
void aomarl_arith_reset(void) { for (int i = 0; i < AR_N; i++) g_arith[i] = 0ULL; }

template <typename T>
static int upload(aomarl_ctx *c, const T *host, size_t n, T **dev) {
  *dev = nullptr;
  if (n == 0) return 0;
  if (!host) return fail("null host array in descriptor");
  void *p = nullptr;
  HIPCHK(hipMalloc(&p, n * sizeof(T)));
  c->owned.push_back(p);
  HIPCHK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
  *dev = (T *)p;
  return 0;
}

// Creation: the plan decides everything on the host (aomarl_create_plan_host.h: the refusals, the DevSys, the tables),
// then each table is one allocation, one copy and one pointer store.  All validation precedes the first HIP call.
int aomarl_create(const aomarl_desc *d, aomarl_ctx **out) {
  if (!d || !out) return fail("aomarl_create: null argument");
  CreatePlan P;
  if (!create_plan(d, P)) return fail("%s", P.msg);
  aomarl_ctx *c = new aomarl_ctx();
  const CreateHost &H = P.host;
  c->sys = P.sys;
  c->nlayers = P.sys.nlayers; c->ndm = P.sys.ndm;
  for (int l = 0; l < c->nlayers; l++) {
    c->dim[l] = H.dim[l]; c->ns[l] = H.ns[l]; c->abclass[l] = H.abclass[l];
    c->deltax[l] = H.deltax[l]; c->deltay[l] = H.deltay[l];
  }
  c->nclass = H.nclass; c->maxdim = H.maxdim; c->maxK = H.maxK; c->small_ok = H.small_ok;
  c->gain = H.gain; c->delay = H.delay;
  c->h_grid = H.h_grid; c->h_prof = H.h_prof; c->h_spupil = H.h_spupil; c->h_tt = H.h_tt;
  c->production_layout = P.production_layout;
  int rc = 0;
  for (size_t i = 0; i < P.tables.size() && !rc; i++) {
    const CreateTable &T = P.tables[i];
    unsigned char *p = nullptr;
    rc = upload<unsigned char>(c, (const unsigned char *)T.data(), T.bytes, &p);
    for (size_t off : T.slots) memcpy((char *)&c->sys + off, &p, sizeof(p));
  }
  if (!rc && P.psf_operand >= 0) {
    // the [hi | lo] split-fp16 form of the frame kernel's PSF operand: per lane 4 floats -> [hi(j = 0..3) | lo(j = 0..3)]
    const CreateTable &T = P.tables[P.psf_operand];
    const float *twf = (const float *)T.data();
    std::vector<_Float16> tw(T.bytes / sizeof(float) * 2);
    for (size_t q = 0; q < T.bytes / sizeof(float) / 4; q++)
      for (int j = 0; j < 4; j++) {
        const float v = twf[q * 4 + j];
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        tw[q * 8 + j] = hi; tw[q * 8 + 4 + j] = lo;
      }
    _Float16 *dev = nullptr;
    rc = upload<_Float16>(c, tw.data(), tw.size(), &dev);
    c->sys.psf_tw_h = dev;
  }
  if (rc) { aomarl_destroy(c); return rc; }
  for (int cls = 0; cls < H.nclass; cls++) {
    const CreateTable &T = P.tables[P.ab_table[cls]];
    c->ab_scale[cls] = gemm_scale((const float *)T.data(), T.bytes / sizeof(float));
  }
  *out = c;
  return 0;
}

int aomarl_destroy(aomarl_ctx *c) {
  if (c)
    for (auto &sg : c->graphs) { (void)hipGraphExecDestroy(sg.exec); (void)hipGraphDestroy(sg.graph); }
  if (c) c->graphs.clear();
  if (!c) return 0;
  for (void *p : c->owned) (void)hipFree(p);
  for (int k = 0; k < 2; k++) {
    if (c->pipe.snap[k]) (void)hipFree(c->pipe.snap[k]);
    if (c->pipe.ev_done[k]) (void)hipEventDestroy(c->pipe.ev_done[k]);
    if (c->pipe.ev_psf[k]) (void)hipEventDestroy(c->pipe.ev_psf[k]);
  }
  if (c->ev_reset) (void)hipEventDestroy(c->ev_reset);
  for (int k = 0; k < 3; k++) if (c->ev_reset2[k]) (void)hipEventDestroy(c->ev_reset2[k]);
  if (c->pipe.ev_cmd) (void)hipEventDestroy(c->pipe.ev_cmd);
  if (c->pipe.ev_commit) (void)hipEventDestroy(c->pipe.ev_commit);
  if (c->pipe.fstream) { (void)hipStreamSynchronize(c->pipe.fstream); (void)hipStreamDestroy(c->pipe.fstream); }
  // the side streams belong to the process (side_stream): drained here, never destroyed
  if (c->atm_stream) (void)hipStreamSynchronize(c->atm_stream);
  if (c->psf_stream) (void)hipStreamSynchronize(c->psf_stream);
  if (c->ev_frame) (void)hipEventDestroy(c->ev_frame);
  if (c->ev_moved) (void)hipEventDestroy(c->ev_moved);
  if (c->ev_psf) (void)hipEventDestroy(c->ev_psf);
  if (c->env_gain) (void)hipFree(c->env_gain);
  if (c->mgain) (void)hipFree(c->mgain);
  if (c->mo) { mo_online_set_owner(c->mo, nullptr); c->mo = nullptr; }      // (not owned: the caller destroys it)
  if (c->mo_mgain_used) (void)hipFree(c->mo_mgain_used);
  if (c->pred) { pred_set_owner(c->pred, nullptr); c->pred = nullptr; }     // (not owned either)
  if (c->seed_stage) (void)hipFree(c->seed_stage);
  rp_free(c);
  if (c->timg) (void)hipFree(c->timg);
  for (hipEvent_t e : c->fw_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->fw_ev_retired) (void)hipEventDestroy(e);
  delete c;
  return 0;
}

static int replace_dev(aomarl_ctx *c, float **slot, const std::vector<float> &h) {
  if (*slot) {
    for (size_t i = 0; i < c->owned.size(); i++)
      if (c->owned[i] == *slot) { c->owned.erase(c->owned.begin() + i); break; }
    (void)hipFree(*slot);
    *slot = nullptr;
  }
  return upload<float>(c, h.data(), h.size(), slot);
}

int aomarl_set_cmat(aomarl_ctx *c, const float *cmat) {
  if (c) c->cfg_epoch++;
  if (!c || !cmat) return fail("aomarl_set_cmat: null argument");
  const int na = c->sys.nactu, nsl = c->sys.nslope;
  const int ld = (nsl + 3) & ~3;
  std::vector<float> h((size_t)na * ld, 0.f);
  for (int r = 0; r < na; r++) memcpy(&h[(size_t)r * ld], cmat + (size_t)r * nsl, sizeof(float) * nsl);
  c->ld_cmat = ld;
  c->cmat_scale = gemm_scale(h.data(), h.size());
  return replace_dev(c, &c->cmat, h);
}

int aomarl_set_slopes2modes(aomarl_ctx *c, int nmodes, const float *s2m) {
  if (c) c->cfg_epoch++;
  if (!c) return fail("aomarl_set_slopes2modes: null ctx");
  if (!s2m) { c->s2m_nmodes = 0; return 0; }                 // dropped (cmat or basis changed)
  if (nmodes < 1) return fail("aomarl_set_slopes2modes: nmodes must be positive");
  const int nsl = c->sys.nslope, ld = (nsl + 3) & ~3;
  std::vector<float> h((size_t)nmodes * ld, 0.f);
  for (int r = 0; r < nmodes; r++) memcpy(&h[(size_t)r * ld], s2m + (size_t)r * nsl, sizeof(float) * nsl);
  int rc = replace_dev(c, &c->s2m, h);
  if (rc) return rc;
  c->s2m_scale = gemm_scale(h.data(), h.size());
  c->s2m_nmodes = nmodes;
  return 0;
}

int aomarl_set_gain(aomarl_ctx *c, float gain) {
  if (c) c->cfg_epoch++;
  if (!c) return fail("null ctx");
  c->gain = gain;
  return 0;
}

int aomarl_set_env_gains(aomarl_ctx *c, const float *gains, int nenv) {
  if (c) c->cfg_epoch++;
  if (!c) return fail("null ctx");
  if (!gains) {                      // back to the scalar gain
    if (c->env_gain) { HIPCHK(hipDeviceSynchronize()); (void)hipFree(c->env_gain); }
    c->env_gain = nullptr; c->env_gain_n = 0;
    return 0;
  }
  if (nenv < 1) return fail("set_env_gains: nenv must be positive");
  if (c->env_gain_n != nenv) {
    if (c->env_gain) { HIPCHK(hipDeviceSynchronize()); (void)hipFree(c->env_gain); c->env_gain = nullptr; }
    HIPCHK(hipMalloc((void **)&c->env_gain, sizeof(float) * (size_t)nenv));
    c->env_gain_n = nenv;
  }
  HIPCHK(hipMemcpy(c->env_gain, gains, sizeof(float) * (size_t)nenv, hipMemcpyHostToDevice));
  return 0;
}

int aomarl_set_modal_gains(aomarl_ctx *c, const float *mgain, int nrows, int nmodes) {
  if (c) c->cfg_epoch++;
  if (!c) return fail("set_modal_gains: null ctx");
  if (c->mo)
    return fail("aomarl_set_modal_gains: an on-line optimiser is attached and owns the gains (aomarl_modopti_online_attach "
                "with NULL first)");
  if (c->pred && !mgain)
    return fail("aomarl_set_modal_gains: a modal predictor is attached and modal gains are what routes every step to its "
                "chain (aomarl_predictor_attach with NULL first)");
  if (c->pipe.active)
    return fail("aomarl_set_modal_gains: a pipelined frame is in flight (aomarl_set_frame_pipeline): the frame pipeline "
                "cannot apply or drop modal gains within an episode -- reset first");
  if (!mgain) {                      // back to the scalar law
    if (c->mgain) { HIPCHK(hipDeviceSynchronize()); (void)hipFree(c->mgain); }
    c->mgain = nullptr; c->mgain_rows = 0; c->mgain_nm = 0; c->h_mgain.clear();
    return 0;
  }
  if (!c->v2m || !c->m2v) return fail("set_modal_gains: no modal basis (aomarl_set_modal)");
  if (nmodes != c->nmodes) return fail("set_modal_gains: nmodes = %d, the modal basis has %d modes", nmodes, c->nmodes);
  if (nrows < 1) return fail("set_modal_gains: nrows = %d: 1 (shared) or one row per environment", nrows);
  const size_t cnt = (size_t)nrows * (size_t)nmodes;
  for (size_t i = 0; i < cnt; i++)
    if (!(mgain[i] >= 0.f) || !isfinite(mgain[i]))
      return fail("set_modal_gains: mgain[%zu][%zu] = %g: entries must be finite and not negative", i / nmodes, i % nmodes, (double)mgain[i]);
  if ((size_t)c->mgain_rows * (size_t)c->mgain_nm != cnt) {
    if (c->mgain) { HIPCHK(hipDeviceSynchronize()); (void)hipFree(c->mgain); c->mgain = nullptr; c->mgain_rows = 0; c->mgain_nm = 0; c->h_mgain.clear(); }
    HIPCHK(hipMalloc((void **)&c->mgain, sizeof(float) * cnt));
  } else {
    HIPCHK(hipDeviceSynchronize());   // a kernel in flight may still read the old values
  }
  c->mgain_rows = nrows; c->mgain_nm = nmodes;
  c->h_mgain.assign(mgain, mgain + cnt);
  HIPCHK(hipMemcpy(c->mgain, mgain, sizeof(float) * cnt, hipMemcpyHostToDevice));
  return 0;
}

int aomarl_get_modal_gains(aomarl_ctx *c, float *mgain_out, int *nrows_out, int *nmodes_out) {
  if (!c) return fail("get_modal_gains: null ctx");
  if (nrows_out) *nrows_out = c->mgain ? c->mgain_rows : 0;
  if (nmodes_out) *nmodes_out = c->mgain ? c->mgain_nm : 0;
  if (mgain_out && c->mgain && c->mo) {        // the applies write the device's copy: read it back
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(c->h_mgain.data(), c->mgain, sizeof(float) * c->h_mgain.size(), hipMemcpyDeviceToHost));
  }
  if (mgain_out && c->mgain) memcpy(mgain_out, c->h_mgain.data(), sizeof(float) * c->h_mgain.size());
  return 0;
}

int aomarl_modopti_online_attach(aomarl_ctx *c, aomarl_state *st, aomarl_modopti_online *m) {
  if (!c) return fail("modopti_online_attach: null ctx");
  c->cfg_epoch++;
  if (!m) {                          // detach: the gains stay as last applied, the host copy follows them
    if (!c->mo) return 0;
    if (c->mgain) {
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipMemcpy(c->h_mgain.data(), c->mgain, sizeof(float) * c->h_mgain.size(), hipMemcpyDeviceToHost));
    }
    mo_online_set_owner(c->mo, nullptr);
    c->mo = nullptr; c->mo_voltage = nullptr;
    if (c->mo_mgain_used) (void)hipFree(c->mo_mgain_used);
    c->mo_mgain_used = nullptr; c->mo_used_stale = false;
    return 0;
  }
  if (!st || !st->voltage) return fail("modopti_online_attach: null state");
  if (c->mo) return fail("modopti_online_attach: an optimiser is attached already (attach NULL first)");
  if (c->pred) return fail("modopti_online_attach: a modal predictor is attached (aomarl_predictor_attach with NULL first): it replaces the integrator whose gains this optimises");
  if (mo_online_owner(m)) return fail("modopti_online_attach: this optimiser is attached to another context");
  if (c->pipe.active)
    return fail("modopti_online_attach: a pipelined frame is in flight (aomarl_set_frame_pipeline): reset first");
  if (!c->mgain) return fail("modopti_online_attach: no modal gains are set (aomarl_set_modal_gains first: the applies write them)");
  if (c->env_gain) return fail("modopti_online_attach: per-environment scalar gains are set (aomarl_set_env_gains): mgain = G / gain needs one gain");
  if (!(c->gain > 0.f) || !isfinite(c->gain)) return fail("modopti_online_attach: gain = %g: mgain = G / gain needs a positive gain", (double)c->gain);
  int nenv, nm, rows;
  mo_online_dims(m, &nenv, &nm, &rows);
  if (nm != c->nmodes || nm != c->mgain_nm) return fail("modopti_online_attach: nmodes = %d, the modal basis has %d modes, the modal gains %d", nm, c->nmodes, c->mgain_nm);
  if (nenv != st->nenv) return fail("modopti_online_attach: nenv = %d, the state has %d environments", nenv, st->nenv);
  if (c->mgain_rows != rows)
    return fail("modopti_online_attach: mgain_rows = %d does not match pool (%d row%s: 1 for pooled gains, nenv otherwise)", c->mgain_rows, rows, rows == 1 ? "" : "s");
  const size_t cnt = (size_t)c->mgain_rows * (size_t)c->mgain_nm;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMalloc((void **)&c->mo_mgain_used, sizeof(float) * cnt));
  HIPCHK(hipMemcpy(c->mo_mgain_used, c->mgain, sizeof(float) * cnt, hipMemcpyDeviceToDevice));
  c->mo_used_stale = false;
  mo_online_set_owner(m, c);
  c->mo = m; c->mo_voltage = st->voltage;
  return 0;
}

int aomarl_predictor_attach(aomarl_ctx *c, aomarl_state *st, aomarl_predictor *p) {
  if (!c) return fail("predictor_attach: null ctx");
  c->cfg_epoch++;
  if (!p) {                          // detach: the command stays as the last frame left it
    if (!c->pred) return 0;
    pred_set_owner(c->pred, nullptr);
    c->pred = nullptr; c->pred_voltage = nullptr;
    return 0;
  }
  if (!st || !st->voltage) return fail("predictor_attach: null state");
  if (c->pred) return fail("predictor_attach: a predictor is attached already (attach NULL first)");
  if (pred_owner(p)) return fail("predictor_attach: this predictor is attached to another context");
  if (c->pipe.active) return fail("predictor_attach: a pipelined frame is in flight (aomarl_set_frame_pipeline): reset first");
  if (c->mo) return fail("predictor_attach: an on-line modal-gain optimiser is attached (aomarl_modopti_online_attach with NULL first)");
  if (!c->mgain) return fail("predictor_attach: no modal gains are set (aomarl_set_modal_gains first: they route every step to the general chain)");
  if (c->env_gain) return fail("predictor_attach: per-environment scalar gains are set (aomarl_set_env_gains): the predictor replaces the integrator");
  int nenv, nm;
  pred_dims(p, &nenv, &nm);
  if (nm != c->nmodes || nm != c->mgain_nm) return fail("predictor_attach: nmodes = %d, the modal basis has %d modes, the modal gains %d", nm, c->nmodes, c->mgain_nm);
  if (nenv != st->nenv) return fail("predictor_attach: nenv = %d, the state has %d environments", nenv, st->nenv);
  pred_set_owner(p, c);
  c->pred = p; c->pred_voltage = st->voltage;
  return 0;
}

// modal gains are set: do they fit this basis and this state?  (name: the entry point asking)
static int mgain_check(const aomarl_ctx *c, int nenv, const char *name) {
  if (c->mgain_nm != c->nmodes)
    return fail("%s: modal gains were set for %d modes, the basis now has %d (aomarl_set_modal_gains again, or clear them)",
                name, c->mgain_nm, c->nmodes);
  if (c->mgain_rows != 1 && c->mgain_rows != nenv)
    return fail("%s: aomarl_set_modal_gains was given nrows = %d, the state has %d environments (1 or %d rows)", name,
                c->mgain_rows, nenv, nenv);
  return 0;
}

int aomarl_set_modal(aomarl_ctx *c, int nmodes, const float *v2m, const float *m2v,
                     const float *freedom, int nact, const int32_t *amodes) {
  if (c) c->cfg_epoch++;
  if (!c || !v2m || !m2v) return fail("aomarl_set_modal: null argument");
  const int na = c->sys.nactu;
  if (nmodes <= 0 || nmodes > na) return fail("nmodes out of range");
  c->nmodes = nmodes;
  c->ld_v2m = (na + 3) & ~3;
  c->ld_m2v = (nmodes + 3) & ~3;
  std::vector<float> a((size_t)nmodes * c->ld_v2m, 0.f), b((size_t)na * c->ld_m2v, 0.f);
  for (int r = 0; r < nmodes; r++) memcpy(&a[(size_t)r * c->ld_v2m], v2m + (size_t)r * na, sizeof(float) * na);
  for (int r = 0; r < na; r++) memcpy(&b[(size_t)r * c->ld_m2v], m2v + (size_t)r * nmodes, sizeof(float) * nmodes);
  int rc = replace_dev(c, &c->v2m, a);
  if (rc) return rc;
  rc = replace_dev(c, &c->m2v, b);
  if (rc) return rc;
  c->v2m_scale = gemm_scale(a.data(), a.size());
  c->m2v_scale = gemm_scale(b.data(), b.size());
  std::vector<float> f(nmodes, 0.f);
  if (freedom) memcpy(f.data(), freedom, sizeof(float) * nmodes);
  rc = replace_dev(c, &c->freedom, f);
  if (rc) return rc;
  c->nact = 0;
  if (nact > 0) {
    if (!amodes) return fail("action_modes is null");
    for (int j = 0; j < nact; j++)
      if (amodes[j] < 0 || amodes[j] >= nmodes) return fail("action mode %d out of range", amodes[j]);
    if (c->amodes) {
      for (size_t i = 0; i < c->owned.size(); i++)
        if (c->owned[i] == c->amodes) { c->owned.erase(c->owned.begin() + i); break; }
      (void)hipFree(c->amodes);
      c->amodes = nullptr;
    }
    rc = upload<int32_t>(c, amodes, nact, &c->amodes);
    if (rc) return rc;
    if (c->amode_inv) {
      for (size_t i = 0; i < c->owned.size(); i++)
        if (c->owned[i] == c->amode_inv) { c->owned.erase(c->owned.begin() + i); break; }
      (void)hipFree(c->amode_inv);
      c->amode_inv = nullptr;
    }
    std::vector<int32_t> inv(nmodes, -1);
    for (int j = 0; j < nact; j++) {
      if (inv[amodes[j]] != -1) return fail("action mode %d listed twice", amodes[j]);
      inv[amodes[j]] = j;
    }
    rc = upload<int32_t>(c, inv.data(), inv.size(), &c->amode_inv);
    if (rc) return rc;
    c->nact = nact;
  }
  return 0;
}

// ---- workspace layout (floats)
struct Work {
  size_t Z, Z2, NEWL, ZREF, ZREF2, MODES, TR, TPART, PEND, GEMM, GEMM_ATM, gemm_floats, total;
  int ldz, ldn, ldm, nblk;
};

static Work work_layout(const aomarl_ctx *c, int nenv) {
  Work w;
  const DevSys &s = c->sys;
  const size_t ncol = (size_t)nenv * (c->nlayers > 0 ? c->nlayers : 1);
  w.ldz = (c->maxK + 3) & ~3;
  w.ldn = (c->maxdim + 3) & ~3;
  w.ldm = (s.nactu + 3) & ~3;
  const int W = 2 * s.hw, RB = 256 / W;
  w.nblk = (s.pupdiam + RB - 1) / RB;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += (n + 3) & ~(size_t)3; return r; };
  w.Z = take(ncol * w.ldz);
  w.NEWL = take(ncol * w.ldn);
  w.ZREF = take(ncol);
  w.Z2 = take(ncol * w.ldz);       // the fused scatter + gather writes the NEXT round's operand while this round's is in use
  w.ZREF2 = take(ncol);
  w.MODES = take((size_t)nenv * w.ldm);
  w.TR = take((size_t)nenv * s.pupdiam * W * 2);
  w.TPART = take((size_t)nenv * w.nblk * 4);
  w.PEND = take((size_t)nenv * (W * W + 4));
  {
    size_t mn = std::max(ncol * (size_t)w.ldn, (size_t)nenv * (size_t)w.ldm);
    w.gemm_floats = 8 * mn;            // up to 8 partial tiles of the split-K GEMM
    w.GEMM = take(w.gemm_floats);
    w.GEMM_ATM = take(w.gemm_floats);  // the extrusion's own split-K workspace: it may run on the side stream
  }
  w.total = o;
  return w;
}

size_t aomarl_workspace_floats(const aomarl_ctx *c, int nenv) {
  return c ? work_layout(c, nenv).total : 0;
}
size_t aomarl_screen_stride(const aomarl_ctx *c) { return c ? (size_t)c->sys.screen_stride : 0; }
size_t aomarl_dmshape_stride(const aomarl_ctx *c) { return c ? (size_t)c->sys.shape_stride : 0; }

static int check_range(const aomarl_ctx *c, const aomarl_state *st, int b, int n) {
  if (!c || !st) return fail("null ctx/state");
  if (c->pipe.active && !c->pipe_internal && st->screens == c->pipe.owner_screens)
    return fail("a pipelined frame is in flight on this state (aomarl_set_frame_pipeline): only aomarl_env_step and a "
                "full-range aomarl_reset are accepted until the reset -- slopes / voltage of odd frames are in the twin, "
                "the screens a frame ahead");
  if (b < 0 || n < 0 || b + n > st->nenv) return fail("env range [%d, %d) outside [0, %d)", b, b + n, st->nenv);
  if (st->ld_actu < c->sys.nactu) return fail("ld_actu (%d) < nactu (%d)", st->ld_actu, c->sys.nactu);
  if (!st->screens || !st->origin || !st->seeds || !st->ext_count || !st->com || !st->com1 ||
      !st->com2 || !st->err || !st->voltage || !st->slopes || !st->dm_shape || !st->strehl ||
      !st->le_img || !st->frame || !st->work)
    return fail("aomarl_state has a null mandatory buffer");
  return 0;
}

DevState dev_state(const aomarl_state *st) {
  DevState d;
  d.nenv = st->nenv; d.ld_actu = st->ld_actu;
  d.screens = st->screens; d.origin = st->origin; d.seeds = st->seeds; d.ext_count = st->ext_count;
  d.com = st->com; d.com1 = st->com1; d.com2 = st->com2; d.err = st->err; d.voltage = st->voltage;
  d.slopes = st->slopes; d.dm_shape = st->dm_shape; d.bincube = st->bincube;
  d.wfs_phase = st->wfs_phase; d.tar_phase = st->tar_phase; d.strehl = st->strehl;
  d.le_img = st->le_img; d.frame = st->frame; d.work = st->work;
  d.origin_snap = nullptr;
  return d;
}

#include "aomarl_capi_atmos.hip"
#include "aomarl_capi_stages.hip"
#include "aomarl_capi_agents.hip"
#include "aomarl_capi_step.hip"
#include "aomarl_capi_extras.hip"
#include "aomarl_capi_composites.hip"

// ---------------------------------------------------------------- the context as the sensing and field units see it
// (aomarl_env_host.h; they are translation units of their own and never see struct aomarl_ctx)
EnvView env_view(const aomarl_ctx *c) {
  EnvView v;
  v.sys = traced_sys(c);
  v.nlayers = c->nlayers; v.ndm = c->ndm; v.delay = c->delay;
  v.frac_x = c->subpixel_flow ? c->frac_x : nullptr;
  v.frac_y = c->subpixel_flow ? c->frac_y : nullptr;
  return v;
}

int env_busy(const aomarl_ctx *c) {
  return (c->pipe.active ? ENV_PIPELINED : 0) | (c->rp && c->rp->n > 0 ? ENV_RESET_PREFETCHED : 0);
}

int env_refuse_busy(const char *who, const aomarl_ctx *c) {
  const int busy = env_busy(c);
  if (busy & ENV_PIPELINED) return fail("%s: the frame pipeline is on (the frames run a step ahead of the chains)", who);
  if (busy & ENV_RESET_PREFETCHED) return fail("%s: a prefetched reset is in flight", who);
  return 0;
}

int env_trace_ready(aomarl_ctx *c, aomarl_state *st, int b, int n, int flags, void *stream) {
  int rc = check_range(c, st, b, n);
  if (rc) return rc;
  rc = atmos_wait_pending(c, stream);
  if (rc) return rc;
  if (n > 0 && c->defer_dm_shape && (flags & AOMARL_TRACE_DMS))   // the stack-array shapes exist only as voltages: form them
    rc = dm_shape_impl(c, st, b, n, nullptr, false, stream);
  return rc;
}

int launch_inc_u32(uint32_t *p, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_inc_u32, dim3((n + 255) / 256), dim3(256), 0, s, p, n);
  LAUNCHCHK();
  return 0;
}
