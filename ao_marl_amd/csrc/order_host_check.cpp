// order_host_check.cpp -- a stand-alone host program around aomarl_order_host.h (the ledger of a context's side
// streams), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o order_host_check order_host_check.cpp
// No GPU, no HIP.  A breadth-first walk from the freshly constructed ledger: from every reachable state every call below,
// with every argument that matters, under the condition its call site in the library puts in front of it (a refusal,
// or side_stream() having created the handles: `made`, kept beside the ledger; before that every handle is null).
// Streams and events are symbolic handles, the queue is a fixed array.  Required on every edge:
//   - no wait or record on a null handle;
//   - move_join issues exactly one wait, on ev_moved, when a move is pending and the side streams are not joined, and
//     nothing otherwise;
//   - behind prefetch_end the move is pending, frame_wait_pending and screens_dirty_main are false;
//   - behind pipe_move_end no older frame is known; need_prev never stands without one;
//   - a copy of the ledger taken in front of the call, assigned back behind it, gives the state in front of it.
// Exit status 0: all held, every call occurred, and the line "order_host_check: ok (<states> states, <edges> edges)".
//     order_host_check --table     also prints one line per edge: state | call | ops | result | successor
//                                  (tests/test_order_plan.py compares each with the rules as the call sites spelled them)
#include "aomarl_order_host.h"
#include <stdio.h>
#include <string.h>
#include <unordered_map>
#include <string>
#include <vector>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

// a handle is the address of its name
static char MAIN[] = "main", ATM[] = "atm", PSF[] = "psf", OTHER[] = "other", FSTREAM[] = "fstream";
static char EV_FRAME[] = "ev_frame", EV_MOVED[] = "ev_moved", EV_PSF[] = "ev_psf", EV_FORK[] = "ev_fork";
static char EV_DONE0[] = "ev_done0", EV_DONE1[] = "ev_done1", EV_TIMED[] = "ev_timed";
static char SCR_A[] = "A", SCR_B[] = "B";
static const char *nm(const void *h) { return h ? (const char *)h : "-"; }

struct ArrayQueue {
  struct Op { char kind; void *stream, *event; } ops[8];
  int n = 0;
  int wait(void *s, void *e) { if (n >= 8) return 1; ops[n++] = {'w', s, e}; return 0; }
  int record(void *e, void *s) { if (n >= 8) return 1; ops[n++] = {'r', s, e}; return 0; }
};

struct Walked { SideOrder o; bool made = false; };

static std::string key(const Walked &w) {
  char buf[256];
  const SideOrder &o = w.o;
  snprintf(buf, sizeof(buf), "pm=%d scr=%s b=%d n=%d fwp=%d dirty=%d joined=%d fork=%d marked=%d cur=%s prev=%s need=%d psf=%d made=%d",
           o.premoved, nm(o.pre_screens), o.pre_b, o.pre_n, o.frame_wait_pending, o.screens_dirty_main, o.side_joined,
           o.fork_recorded, o.frame_marked, nm(o.ev_frame_cur), nm(o.ev_frame_prev), o.need_prev, o.psf_side, w.made);
  return buf;
}

static bool same(const SideOrder &a, const SideOrder &b) {
  return a.premoved == b.premoved && a.pre_screens == b.pre_screens && a.pre_b == b.pre_b && a.pre_n == b.pre_n &&
         a.frame_wait_pending == b.frame_wait_pending && a.screens_dirty_main == b.screens_dirty_main &&
         a.side_joined == b.side_joined && a.fork_recorded == b.fork_recorded && a.frame_marked == b.frame_marked &&
         a.ev_frame_cur == b.ev_frame_cur && a.ev_frame_prev == b.ev_frame_prev && a.need_prev == b.need_prev &&
         a.psf_side == b.psf_side;
}

enum Call { PSF_JOIN, MOVE_JOIN, RING_WRITE, SCREENS_WRITTEN, PREFETCH_BEGIN, PREFETCH_END, TAKE_MOVE, RESET_RANGE, QUERIES,
            FRAME_LAUNCHED, PSF_FINISH_LAUNCHED, CAPTURE_FORK, PIPE_PREFETCH_BEGIN, PIPE_MOVE_END, FRAME_TAKES_MOVE,
            PIPE_ADOPTS_PLAIN_FRAME, GRAPH_JOIN_OUTSIDE, REPLAYED, CAPTURE_BEGIN, CAPTURE_JOIN, NCALLS };

int main(int argc, char **argv) {
  const bool table = argc >= 2 && !strcmp(argv[1], "--table");
  void *const streams[3] = {MAIN, ATM, OTHER};
  const void *const screens[2] = {SCR_A, SCR_B};
  const int ranges[4][2] = {{0, 4}, {0, 2}, {2, 2}, {1, 2}};      // (b, n): the batch, its halves, its middle
  std::unordered_map<std::string, int> seen;
  std::vector<Walked> todo;
  unsigned long long nedges = 0, ncall[NCALLS] = {0};
  todo.push_back(Walked());
  seen[key(todo[0])] = 0;

  for (size_t at = 0; at < todo.size(); at++) {
    const Walked from = todo[at];
    const std::string from_key = key(from);
    // one edge: the call's text, then what it did to a copy of the state
    Walked w;
    ArrayQueue q;
    char call[96], result[160];
    auto begin = [&]() { w = from; q.n = 0; strcpy(result, "-"); };
    auto create = [&]() { if (!w.made) { w.o.handles_created(EV_FRAME); w.made = true; } };     // side_stream()
    auto H = [&](void *h) -> void * { return w.made ? h : nullptr; };
    auto end = [&](Call which) -> int {
      nedges++; ncall[which]++;
      for (int i = 0; i < q.n; i++) REQUIRE(q.ops[i].stream && q.ops[i].event);
      const SideOrder &o = w.o;
      REQUIRE(!o.need_prev || o.ev_frame_prev);
      REQUIRE(!o.premoved || o.pre_screens);
      if (which == MOVE_JOIN) {
        if (from.o.premoved && !from.o.side_joined) REQUIRE(q.n == 1 && q.ops[0].kind == 'w' && q.ops[0].event == EV_MOVED);
        else REQUIRE(q.n == 0);
      }
      if (which == PREFETCH_END) REQUIRE(o.premoved && !o.frame_wait_pending && !o.screens_dirty_main);
      if (which == PIPE_MOVE_END) REQUIRE(!o.ev_frame_prev && !o.need_prev && !o.older_frame_in_flight());
      { SideOrder back = w.o; const SideOrder snap = from.o; back = snap; REQUIRE(same(back, from.o)); }
      const std::string to = key(w);
      if (seen.emplace(to, (int)todo.size()).second) todo.push_back(w);
      if (table) {
        printf("%s | %s |", from_key.c_str(), call);
        for (int i = 0; i < q.n; i++)
          if (q.ops[i].kind == 'w') printf(" wait(%s,%s)", nm(q.ops[i].stream), nm(q.ops[i].event));
          else printf(" record(%s,%s)", nm(q.ops[i].event), nm(q.ops[i].stream));
        if (!q.n) printf(" -");
        printf(" | %s | %s\n", result, to.c_str());
      }
      return 0;
    };
#define EDGE(which) do { if (end(which)) return 1; } while (0)

    for (void *s : streams) {
      if (s == ATM && !from.made) continue;                        // nobody has that handle yet
      begin(); snprintf(call, sizeof(call), "psf_join(%s)", nm(s));
      REQUIRE(w.o.psf_join(q, s, H(EV_PSF)) == 0); EDGE(PSF_JOIN);
      begin(); snprintf(call, sizeof(call), "move_join(%s)", nm(s));
      REQUIRE(w.o.move_join(q, s, H(EV_MOVED)) == 0); EDGE(MOVE_JOIN);
      for (int overlap = 0; overlap < 2; overlap++) {
        begin(); snprintf(call, sizeof(call), "ring_write(%s,%d)", nm(s), overlap);
        REQUIRE(w.o.ring_write(q, s, H(ATM), overlap != 0) == 0); EDGE(RING_WRITE);
      }
    }
    begin(); strcpy(call, "screens_written()"); w.o.screens_written(); EDGE(SCREENS_WRITTEN);
    // prefetch_atmos_impl: refused while a move is pending; side_stream() first
    if (!from.o.move_pending())
      for (int reuse = 0; reuse < 2; reuse++)
        for (int capturing = 0; capturing < 2; capturing++) {
          begin(); create(); snprintf(call, sizeof(call), "prefetch_begin(main,%d,%d)", reuse, capturing);
          REQUIRE(w.o.prefetch_begin(q, MAIN, ATM, EV_FRAME, EV_FORK, reuse != 0, capturing != 0) == 0); EDGE(PREFETCH_BEGIN);
        }
    // ... and its end (the same function, or pipe_prefetch behind the same refusal): of the batch or of its first half
    if (from.made && !from.o.move_pending())
      for (int carried = 0; carried < 2; carried++)
        for (int r = 0; r < 2; r++) {
          begin(); snprintf(call, sizeof(call), "prefetch_end(%d,A,%d,%d)", carried, ranges[r][0], ranges[r][1]);
          REQUIRE(w.o.prefetch_end(q, ATM, EV_MOVED, carried != 0, SCR_A, ranges[r][0], ranges[r][1]) == 0); EDGE(PREFETCH_END);
        }
    for (const void *scr : screens)
      for (int r = 0; r < 4; r++) {
        begin(); snprintf(call, sizeof(call), "take_move(%s,%d,%d)", nm(scr), ranges[r][0], ranges[r][1]);
        strcpy(result, w.o.take_move(scr, ranges[r][0], ranges[r][1]) ? "taken" : "not"); EDGE(TAKE_MOVE);
        begin(); snprintf(call, sizeof(call), "reset_range(%s,%d,%d)", nm(scr), ranges[r][0], ranges[r][1]);
        const MoveOverlap v = w.o.reset_range(scr, ranges[r][0], ranges[r][1]);
        if (v == MOVE_OVERLAPS) snprintf(result, sizeof(result), "overlaps [%d, %d)", w.o.moved_b(), w.o.moved_b() + w.o.moved_n());
        else strcpy(result, v == MOVE_NONE ? "none" : v == MOVE_COVERED ? "covered" : "disjoint");
        EDGE(RESET_RANGE);
      }
    {
      begin(); strcpy(call, "queries()");
      void *held[2];
      w.o.held_events(held);
      snprintf(result, sizeof(result), "pending=%d on_A=%d on_B=%d whole_A=%d older=%d steady=%d outstanding=%d held=%s,%s",
               w.o.move_pending(), w.o.move_pending_on(SCR_A), w.o.move_pending_on(SCR_B), w.o.move_is(SCR_A, 0, 4),
               w.o.older_frame_in_flight(), w.o.steady_after_plain(), w.o.outstanding(), nm(held[0]), nm(held[1]));
      EDGE(QUERIES);
    }
    // frame_fused_impl: a pipelined frame or the prefetch off (0), or a plain frame with the prefetch on (side_stream()
    // first) carrying ev_frame or a timing event
    begin(); strcpy(call, "frame_launched(0,-)");
    REQUIRE(w.o.frame_launched(q, false, H(PSF), nullptr) == 0); EDGE(FRAME_LAUNCHED);
    for (void *ev : {(void *)EV_FRAME, (void *)EV_TIMED}) {
      begin(); create(); snprintf(call, sizeof(call), "frame_launched(1,%s)", nm(ev));
      REQUIRE(w.o.frame_launched(q, true, PSF, ev) == 0); EDGE(FRAME_LAUNCHED);
    }
    if (from.made)
      for (int capturing = 0; capturing < 2; capturing++) {
        begin(); snprintf(call, sizeof(call), "psf_finish_launched(%d)", capturing);
        REQUIRE(w.o.psf_finish_launched(q, capturing != 0, EV_PSF, PSF) == 0); EDGE(PSF_FINISH_LAUNCHED);
      }
    begin(); create(); strcpy(call, "capture_fork(main)");
    REQUIRE(w.o.capture_fork(q, EV_FORK, MAIN) == 0); EDGE(CAPTURE_FORK);
    // pipe_prefetch: refused while a move is pending; the two parities, or (first step) the plain frame's mark as the older
    if (from.made && !from.o.move_pending())
      for (int k = 0; k < 3; k++) {
        void *older = k == 0 ? EV_DONE0 : k == 1 ? EV_DONE1 : from.o.frame_mark(), *newest = k == 1 ? EV_DONE0 : EV_DONE1;
        begin(); snprintf(call, sizeof(call), "pipe_prefetch_begin(%s,%s)", k == 2 ? "mark" : nm(older), nm(newest));
        w.o.pipe_prefetch_begin(older, newest); EDGE(PIPE_PREFETCH_BEGIN);
      }
    if (from.made)
      for (int copy = 0; copy < 2; copy++) {
        begin(); snprintf(call, sizeof(call), "pipe_move_end(%d)", copy);
        REQUIRE(w.o.pipe_move_end(q, ATM, copy != 0) == 0); EDGE(PIPE_MOVE_END);
      }
    // pipe_launch_frame: refused unless the move of the whole batch is pending
    if (from.o.move_is(SCR_A, 0, 4)) {
      begin(); strcpy(call, "frame_takes_move()");
      REQUIRE(w.o.frame_takes_move(q, FSTREAM, H(EV_MOVED)) == 0); EDGE(FRAME_TAKES_MOVE);
    }
    // env_step_pipelined, first step: only behind a plain step that left the steady state
    if (from.o.steady_after_plain()) {
      begin(); strcpy(call, "pipe_adopts_plain_frame()");
      snprintf(result, sizeof(result), "%s", nm(w.o.pipe_adopts_plain_frame())); EDGE(PIPE_ADOPTS_PLAIN_FRAME);
    }
    // aomarl_env_step's graph form.  With the prefetch on: only with the move of the whole batch pending, side_stream() first
    if (from.o.move_is(SCR_A, 0, 4)) {
      begin(); create(); strcpy(call, "graph_join_outside(main)");
      REQUIRE(w.o.graph_join_outside(q, MAIN, EV_MOVED, EV_PSF) == 0); EDGE(GRAPH_JOIN_OUTSIDE);
      begin(); strcpy(call, "replayed(1)"); w.o.replayed(true); EDGE(REPLAYED);
    }
    if (!from.o.move_pending()) {                                  // with the prefetch off: only with no move pending
      begin(); strcpy(call, "replayed(0)"); w.o.replayed(false); EDGE(REPLAYED);
    }
    begin(); strcpy(call, "capture_begin()"); w.o.capture_begin(); EDGE(CAPTURE_BEGIN);
    if (from.made) {
      begin(); strcpy(call, "capture_join(main)");
      REQUIRE(w.o.capture_join(q, MAIN, EV_PSF, EV_MOVED) == 0); EDGE(CAPTURE_JOIN);
    }
  }
  for (int k = 0; k < NCALLS; k++) REQUIRE(ncall[k] > 0);
  printf("order_host_check: ok (%zu states, %llu edges)\n", todo.size(), nedges);
  return 0;
}
