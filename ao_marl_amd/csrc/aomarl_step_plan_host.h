// aomarl_step_plan_host.h -- what aomarl_env_step (aomarl_capi_step.hip) decides before it launches anything: which
// chain runs one step.  No HIP include and no global: the facts come in as a plain struct (step_facts in
// aomarl_capi_step.hip is the one place that reads them off the context, the glue and the call's arguments), so the
// stand-alone host program (step_plan_host_check.cpp) walks the same text over every combination of them, also under
// the address and undefined-behaviour sanitizers; tests/golden/step_plans.txt pins the outcome.
//
// The step is head | sense | tail, inside a route:
//
//   fused  = !UNFUSED && exactly one tip-tilt mirror && (deferred DM shape || no other mirror) && !modal gains
//            (the chain in its fused form: every split-K reduction in the kernel that consumes the product)
//   small  = fused && "small_chain" && the sizes fit k_small_head / k_small_tail && cmat && !per-environment gains
//   short  = fused && !small && !denoiser && "residual_shortcut" && s2m for these modes && !per-environment gains
//
//   head   HEAD_STAGES    !fused            rl_control_modes, apply_control, comp_strehl, agent_rewards
//          HEAD_SMALL     small             k_small_head
//          HEAD_FUSED     fused && !small   compose + rewards, m2v slabs, delay line, tip-tilt slot + Strehl commit
//   sense  SENSE_DENOISER denoiser          move, frame -> image cube, denoiser, centroids
//          SENSE_FRAME    otherwise         aomarl_next_part_one without its do_control
//   tail   TAIL_STAGES    !fused                        do_control, aomarl_volts2modes, the state blocks
//          TAIL_FUSED     fused && (denoiser || neither small nor short)
//                                                       do_control, v2m slabs reduced by the state blocks' kernel
//          TAIL_SMALL     small && !denoiser            k_small_tail (do_control, v2m . err, the state blocks)
//          TAIL_SHORTCUT  short                         -(v2m . cmat) . slopes as slabs, the state blocks: NO do_control
//                                                       (the integrator lives in the Btt coordinates, the next head
//                                                       rebuilds the command)
//   route  PIPELINED          fused && !denoiser && !"graph_step" && !capturing && deferred DM shape && every one of
//                             the pipeline's own conditions (StepFacts: twin .. one-pass frame kernel)
//          REFUSED_IN_FLIGHT  not that, but a pipelined frame of this state is in flight: an error, nothing launched
//          PLAIN              otherwise, when !"graph_step" || capturing || modal gains: launched call by call
//          PLAIN_MAY_REPLAY   otherwise: the HIP-graph form, if the caller is in the steady state (decided where the
//                             device-side bookkeeping is, aomarl_env_step)
//
// What follows from it (step_plan_host_check.cpp states these over all combinations):
//   - a denoiser on a small system: HEAD_SMALL with TAIL_FUSED -- the sensing writes slopes by another route, the head
//     is the same product either way;
//   - modal gains (aomarl_set_modal_gains): stages everywhere, PLAIN -- aomarl_rl_control_modes and aomarl_do_control
//     apply them; a law that must "stand aside" goes into `fused` and nowhere else;
//   - UNFUSED forces stages; small wins over the shortcut; the small chain and the shortcut never run unfused;
//   - per-environment gains are refused by the step itself (one scalar gain); here they only keep small and short off,
//     which is what aomarl_env_step_shortcut reports.
#pragma once

// k_small_head / k_small_tail: LDS arrays of these sizes, one workgroup per environment
constexpr int SMALL_NM = 512, SMALL_NA = 512, SMALL_NSL = 1024;
constexpr long long SMALL_CMAT = 65536;      // ... each of which reads the whole command matrix: at most this many entries (nactu x nslope)

struct StepFacts {
  // fused form
  bool unfused;          // glue->flags & AOMARL_ENV_STEP_UNFUSED
  bool one_tt;           // exactly one tip-tilt mirror ...
  bool no_other_dm;      // ... and no other mirror
  bool defer_shape;      // "defer_dm_shape" and the frame kernel can take the stack-array DM from the voltages
  int ktt;               // index of the (last) tip-tilt mirror, -1: none.  Not a decision: kernels take it as an argument
  // gains
  bool mgain, env_gain;  // aomarl_set_modal_gains / aomarl_set_env_gains in force
  // small chain
  bool small_opt;        // "small_chain"
  int nactu, nslope, nmodes;
  bool cmat;
  // residual shortcut
  bool shortcut_opt;     // "residual_shortcut"
  bool s2m_match;        // aomarl_set_slopes2modes given, for the glue's mode count
  bool denoiser;
  // the frame pipeline's own conditions (they count only all together)
  bool twin, pipe_opt, owner;      // a twin is set, "frame_pipeline", the twin belongs to this state
  bool prefetch, delay_one, noiseless, accum, subpixel, frame_fused;   // "prefetch_atmos", delay == 1, noise < 0, wind accumulators given, "subpixel_flow", one-pass frame kernel
  bool in_flight;        // a pipelined frame of this state is in flight
  bool graph_step, capturing;
};

enum StepRoute { PIPELINED, REFUSED_IN_FLIGHT, PLAIN, PLAIN_MAY_REPLAY };
enum HeadKind { HEAD_STAGES, HEAD_FUSED, HEAD_SMALL };
enum SenseKind { SENSE_DENOISER, SENSE_FRAME };
enum TailKind { TAIL_STAGES, TAIL_FUSED, TAIL_SMALL, TAIL_SHORTCUT };

struct StepPlan {
  StepRoute route;
  HeadKind head;
  SenseKind sense;
  TailKind tail;
};

static inline bool step_small_fits(int nactu, int nslope, int nmodes) {
  return nactu <= SMALL_NA && nslope <= SMALL_NSL && nmodes <= SMALL_NM && (long long)nactu * nslope <= SMALL_CMAT;
}

static inline bool tail_runs_do_control(TailKind t) { return t == TAIL_STAGES || t == TAIL_FUSED; }

static inline StepPlan step_plan(const StepFacts &f) {
  const bool fused = !f.unfused && f.one_tt && (f.defer_shape || f.no_other_dm) && !f.mgain;
  const bool small = fused && f.small_opt && step_small_fits(f.nactu, f.nslope, f.nmodes) && f.cmat && !f.env_gain;
  const bool shortcut = fused && !small && !f.denoiser && f.shortcut_opt && f.s2m_match && !f.env_gain;
  const bool pipelined = fused && !f.denoiser && !f.graph_step && !f.capturing && f.defer_shape && f.twin && f.pipe_opt &&
                         f.owner && f.prefetch && f.delay_one && f.noiseless && f.accum && !f.subpixel && f.frame_fused;
  StepPlan p;
  p.head = !fused ? HEAD_STAGES : small ? HEAD_SMALL : HEAD_FUSED;
  p.sense = f.denoiser ? SENSE_DENOISER : SENSE_FRAME;
  p.tail = !fused ? TAIL_STAGES : shortcut ? TAIL_SHORTCUT : (small && !f.denoiser) ? TAIL_SMALL : TAIL_FUSED;
  p.route = pipelined ? PIPELINED
          : f.in_flight ? REFUSED_IN_FLIGHT
          : (!f.graph_step || f.capturing || f.mgain) ? PLAIN : PLAIN_MAY_REPLAY;
  return p;
}

// the delay line: voltage = wa com + wb com1 + wc com2 (k_delay; com1 / com2: the commands of one / two frames ago).
// ahead: evaluated one frame ahead (the voltages of the frame that follows the one in flight): shifted by one command.
struct DelayWeights { float wa, wb, wc; };
static inline DelayWeights delay_weights(float delay, bool ahead) {
  DelayWeights w = delay <= 1.f ? DelayWeights{1.f - delay, delay, 0.f} : DelayWeights{0.f, 2.f - delay, delay - 1.f};
  if (ahead) w = DelayWeights{w.wb, w.wc, 0.f};
  return w;
}
