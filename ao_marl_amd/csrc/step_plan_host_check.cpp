// step_plan_host_check.cpp -- a stand-alone host program around aomarl_step_plan_host.h (which chain aomarl_env_step
// runs), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o step_plan_host_check step_plan_host_check.cpp
// No GPU, no HIP.  It walks every combination of the boolean facts (the sizes as "fit" / "do not fit") and requires what
// the header's comment promises of the plan; the size rule and the delay weights at their boundaries.  Exit status 0:
// all held, and the line "step_plan_host_check: ok (<count> combinations)".
//     step_plan_host_check --table     also prints the plan itself (tests/test_step_plan.py compares it with
//                                      tests/golden/step_plans.txt): one line per combination of the facts that decide
//                                      head, sense and tail; one line per combination of what the route depends on,
//                                      with the pipeline's own conditions all holding, and with each one alone failing
#include "aomarl_step_plan_host.h"
#include <stdio.h>
#include <string.h>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

// the facts that decide head, sense and tail (bits 0..11), then what else the route depends on (12..14), then the
// pipeline's own conditions (15..23; subpixel counts inverted: every bit set = every condition holds)
static const char *const kNames[24] = {"unfused", "one_tt", "no_other_dm", "defer_shape", "mgain", "env_gain", "small_opt", "fits",
                                       "cmat", "shortcut_opt", "s2m_match", "denoiser", "in_flight", "graph_step", "capturing",
                                       "twin", "pipe_opt", "owner", "prefetch", "delay_one", "noiseless", "accum", "!subpixel", "frame_fused"};
enum { CHAIN_BITS = 12, ROUTE_BITS = 3, PIPE_BITS = 9, ALL_BITS = CHAIN_BITS + ROUTE_BITS + PIPE_BITS };
static const unsigned PIPE_ALL = ((1u << PIPE_BITS) - 1) << (CHAIN_BITS + ROUTE_BITS);

static StepFacts facts(unsigned b) {
#define bit(k) (((b >> (k)) & 1u) != 0)
  StepFacts f;
  f.unfused = bit(0); f.one_tt = bit(1); f.no_other_dm = bit(2); f.defer_shape = bit(3); f.ktt = f.one_tt ? 1 : -1;
  f.mgain = bit(4); f.env_gain = bit(5); f.small_opt = bit(6);
  f.nactu = bit(7) ? 90 : SMALL_NA + 1; f.nslope = 152; f.nmodes = 85;
  f.cmat = bit(8); f.shortcut_opt = bit(9); f.s2m_match = bit(10); f.denoiser = bit(11);
  f.in_flight = bit(12); f.graph_step = bit(13); f.capturing = bit(14);
  f.twin = bit(15); f.pipe_opt = bit(16); f.owner = bit(17); f.prefetch = bit(18); f.delay_one = bit(19);
  f.noiseless = bit(20); f.accum = bit(21); f.subpixel = !bit(22); f.frame_fused = bit(23);
  return f;
#undef bit
}

static const char *const kRoute[] = {"PIPELINED", "REFUSED_IN_FLIGHT", "PLAIN", "PLAIN_MAY_REPLAY"};
static const char *const kHead[] = {"HEAD_STAGES", "HEAD_FUSED", "HEAD_SMALL"};
static const char *const kSense[] = {"SENSE_DENOISER", "SENSE_FRAME"};
static const char *const kTail[] = {"TAIL_STAGES", "TAIL_FUSED", "TAIL_SMALL", "TAIL_SHORTCUT"};

int main(int argc, char **argv) {
  const bool table = argc >= 2 && !strcmp(argv[1], "--table");
  // ---- the size rule and the delay weights
  REQUIRE(step_small_fits(SMALL_NA, 128, SMALL_NM) && !step_small_fits(SMALL_NA + 1, 1, 1));
  REQUIRE(step_small_fits(64, SMALL_NSL, 1) && !step_small_fits(1, SMALL_NSL + 1, 1) && !step_small_fits(65, SMALL_NSL, 1));
  REQUIRE(!step_small_fits(1, 1, SMALL_NM + 1) && step_small_fits(256, 256, 1) && !step_small_fits(257, 256, 1));
  REQUIRE(step_small_fits(90, 152, 85));
  const struct { float d; bool ahead; float wa, wb, wc; } dw[] = {
      {0.f, false, 1.f, 0.f, 0.f}, {0.25f, false, 0.75f, 0.25f, 0.f}, {1.f, false, 0.f, 1.f, 0.f}, {1.75f, false, 0.f, 0.25f, 0.75f},
      {2.f, false, 0.f, 0.f, 1.f}, {1.f, true, 1.f, 0.f, 0.f}, {0.25f, true, 0.25f, 0.f, 0.f}, {1.75f, true, 0.25f, 0.75f, 0.f}};
  for (const auto &t : dw) {
    const DelayWeights w = delay_weights(t.d, t.ahead);
    REQUIRE(w.wa == t.wa && w.wb == t.wb && w.wc == t.wc);
  }
  // ---- every combination
  unsigned long long count = 0, seen_route[4] = {0, 0, 0, 0}, seen_head[3] = {0, 0, 0}, seen_tail[4] = {0, 0, 0, 0};
  static StepPlan chain[1u << CHAIN_BITS];        // the plans of the chain's facts alone
  for (unsigned b = 0; b < (1u << CHAIN_BITS); b++) chain[b] = step_plan(facts(b));
  for (unsigned b = 0; b < (1u << ALL_BITS); b++) {
    const StepFacts f = facts(b);
    const StepPlan p = step_plan(f);
    const bool fused_head = p.head != HEAD_STAGES;
    const bool pipe_conditions = (b & PIPE_ALL) == PIPE_ALL;
    count++; seen_route[p.route]++; seen_head[p.head]++; seen_tail[p.tail]++;
    // head and tail are both staged or both fused
    REQUIRE(fused_head == (p.tail != TAIL_STAGES));
    REQUIRE(p.tail != TAIL_SMALL || p.head == HEAD_SMALL);
    if (p.tail == TAIL_SHORTCUT || p.tail == TAIL_SMALL) REQUIRE(fused_head && !f.denoiser && !f.env_gain);
    if (p.route == PIPELINED) REQUIRE(fused_head && !f.denoiser && !f.mgain && !f.graph_step && !f.capturing && pipe_conditions && f.defer_shape);
    if (f.mgain) REQUIRE(p.head == HEAD_STAGES && p.tail == TAIL_STAGES && p.route != PIPELINED && p.route != PLAIN_MAY_REPLAY);
    if (f.unfused) REQUIRE(p.head == HEAD_STAGES && p.tail == TAIL_STAGES);
    REQUIRE((p.sense == SENSE_DENOISER) == f.denoiser);
    if (p.sense == SENSE_DENOISER) REQUIRE(tail_runs_do_control(p.tail));
    REQUIRE(tail_runs_do_control(p.tail) == (p.tail == TAIL_STAGES || p.tail == TAIL_FUSED));
    // a denoiser changes the tail only: the head is what it is without one
    REQUIRE(chain[b & ((1u << CHAIN_BITS) - 1) & ~(1u << 11)].head == p.head);
    // small wins over the shortcut
    if (fused_head && !f.denoiser && !f.env_gain && f.small_opt && f.cmat && step_small_fits(f.nactu, f.nslope, f.nmodes)) REQUIRE(p.tail == TAIL_SMALL);
    if (p.tail == TAIL_SHORTCUT) REQUIRE(p.head == HEAD_FUSED && f.shortcut_opt && f.s2m_match);
    if (p.head == HEAD_SMALL) REQUIRE(f.small_opt && f.cmat && step_small_fits(f.nactu, f.nslope, f.nmodes));
    // the refusal: only with a frame in flight and a call the pipeline does not take; never silently plain then
    REQUIRE((p.route == REFUSED_IN_FLIGHT) == (f.in_flight && p.route != PIPELINED));
    if (p.route == PLAIN_MAY_REPLAY) REQUIRE(f.graph_step && !f.capturing);
    if (p.route == PLAIN && !f.mgain) REQUIRE(!f.graph_step || f.capturing);
    // head, sense and tail depend on the first CHAIN_BITS facts alone; the route on `fused`, the denoiser and the rest
    { const StepPlan &q = chain[b & ((1u << CHAIN_BITS) - 1)]; REQUIRE(q.head == p.head && q.sense == p.sense && q.tail == p.tail); }
  }
  for (int k = 0; k < 4; k++) REQUIRE(seen_route[k] > 0 && seen_tail[k] > 0);
  for (int k = 0; k < 3; k++) REQUIRE(seen_head[k] > 0);
  if (table) {
    printf("# chain:");
    for (int k = 0; k < CHAIN_BITS; k++) printf(" %s", kNames[k]);
    printf(" -> head sense tail\n");
    for (unsigned b = 0; b < (1u << CHAIN_BITS); b++) {
      const StepPlan p = step_plan(facts(b));
      for (int k = 0; k < CHAIN_BITS; k++) putchar('0' + ((b >> k) & 1u));
      printf(" %s %s %s\n", kHead[p.head], kSense[p.sense], kTail[p.tail]);
    }
    // the route: of the chain's facts it sees unfused, one_tt, no_other_dm, defer_shape, mgain (through `fused`) and the
    // denoiser -- required here: the other six change nothing
    const int rbits[9] = {0, 1, 2, 3, 4, 11, 12, 13, 14};
    printf("# route:");
    for (int k : rbits) printf(" %s", kNames[k]);
    printf(" -> the pipeline's own conditions (");
    for (int k = CHAIN_BITS + ROUTE_BITS; k < ALL_BITS; k++) printf("%s%s", kNames[k], k + 1 < ALL_BITS ? ", " : "");
    printf(") all hold | each one alone fails\n");
    for (unsigned r = 0; r < (1u << 9); r++) {
      unsigned b = 0;
      for (int k = 0; k < 9; k++) b |= ((r >> k) & 1u) << rbits[k];
      const StepRoute all = step_plan(facts(b | PIPE_ALL)).route;
      const StepRoute one = step_plan(facts((b | PIPE_ALL) & ~(1u << (CHAIN_BITS + ROUTE_BITS)))).route;
      for (int k = CHAIN_BITS + ROUTE_BITS; k < ALL_BITS; k++) REQUIRE(step_plan(facts((b | PIPE_ALL) & ~(1u << k))).route == one);
      for (unsigned o = 0; o < (1u << CHAIN_BITS); o++) {          // the chain's other facts
        if (o & 0x81Fu) continue;
        REQUIRE(step_plan(facts(b | o | PIPE_ALL)).route == all && step_plan(facts((b | o | PIPE_ALL) & ~(1u << 20))).route == one);
      }
      for (int k = 0; k < 9; k++) putchar('0' + ((r >> k) & 1u));
      printf(" %s | %s\n", kRoute[all], kRoute[one]);
    }
  }
  printf("step_plan_host_check: ok (%llu combinations)\n", count);
  return 0;
}
