// aomarl_order_host.h -- how a context's side streams are ordered against the caller's stream: one ledger (SideOrder)
// and the transitions that change it.  No HIP include and no global: streams and events are opaque handles the
// context owns (the ledger never creates or destroys one), and every wait and record goes through a queue argument
//     int wait(void *stream, void *event);      int record(void *event, void *stream);      (0, or the project's error)
// which in the library is HipOrderQueue (aomarl_capi_atmos.hip, over hipStreamWaitEvent / hipEventRecord) and in the
// stand-alone host program (order_host_check.cpp) a fixed array: that program walks every reachable state of the
// ledger under the address and undefined-behaviour sanitizers, and tests/test_order_plan.py compares every edge with
// the rules as they stood at their call sites before there was a ledger.  A transition that fails leaves the fields it
// had not reached yet as they were (what the call sites did).
//
// The streams: the caller's ("main"), the extrusion stream (atm: the prefetched move of the next frame), the PSF
// stream (psf: the second axis of the PSF window), the frame pipeline's own (FramePipe, not kept here).
// The events ("Stream ordering", has the table): ev_frame or a timed launch's closing event = "the readers
// of the screens are done" (frame_mark); ev_moved = "the prefetched move is done"; ev_psf = "the PSF finish on the
// side stream is done"; ev_fork = where the side streams enter a graph capture.
#pragma once

enum MoveOverlap { MOVE_NONE, MOVE_COVERED, MOVE_DISJOINT, MOVE_OVERLAPS };

struct SideOrder {
  // a prefetched move is pending, of environments [pre_b, pre_b + pre_n) of the state with these screens
  bool premoved = false;
  const void *pre_screens = nullptr;
  int pre_b = 0, pre_n = 0;
  // the extrusion stream has not yet waited for the frame that reads the screens: its first ring write does
  bool frame_wait_pending = false;
  bool screens_dirty_main = true;       // the screens / origins were last written on the caller's stream
  bool side_joined = false;             // the caller's stream has waited for everything issued on the side streams
  bool fork_recorded = false;           // this capture has recorded ev_fork
  // the event the screens' readers were last marked with, and: nothing was launched on that stream since
  bool frame_marked = false;
  void *ev_frame_cur = nullptr;
  // a pipelined prefetch, between its begin and its end: the OLDER frame in flight, and nobody has waited for it yet
  void *ev_frame_prev = nullptr;
  bool need_prev = false;
  bool psf_side = false;                // a PSF finish launched on the side stream may still run

  // ---- queries
  bool move_pending() const { return premoved; }
  bool move_pending_on(const void *screens) const { return premoved && pre_screens == screens; }
  bool move_is(const void *screens, int b, int n) const { return move_pending_on(screens) && pre_b == b && pre_n == n; }
  int moved_b() const { return pre_b; }
  int moved_n() const { return pre_n; }
  bool older_frame_in_flight() const { return ev_frame_prev != nullptr; }
  void *frame_mark() const { return ev_frame_cur; }
  // a plain step left the steady state behind: its move prefetched, its PSF finish on the side stream
  bool steady_after_plain() const { return premoved && psf_side; }
  // a prefetched move or a pipelined prefetch is outstanding (what a change of the atmosphere would have to ask)
  bool outstanding() const { return premoved || ev_frame_prev != nullptr; }
  // the events a frame in flight may still be known by: not to be re-recorded by anybody else
  void held_events(void *out[2]) const { out[0] = ev_frame_cur; out[1] = ev_frame_prev; }

  // the side handles were created: until a frame says otherwise the readers' mark is ev_frame
  void handles_created(void *ev_frame) { ev_frame_cur = ev_frame; }

  // whoever reads or overwrites the pending PSF window on `stream` is behind a finish still on the side stream
  template <class Q> int psf_join(Q &q, void *stream, void *ev_psf) {
    if (psf_side && !side_joined) { int rc = q.wait(stream, ev_psf); if (rc) return rc; }
    psf_side = false;
    return 0;
  }
  // whoever touches the screens on `stream` is behind a prefetched move still on the extrusion stream
  template <class Q> int move_join(Q &q, void *stream, void *ev_moved) const {
    if (premoved && !side_joined) return q.wait(stream, ev_moved);
    return 0;
  }
  // the first kernel of a move that WRITES ring lines on s: on the extrusion stream it is behind the readers of the
  // screens -- the OLDER frame in flight when the group may run beside the newest (overlap), else the newest; on any
  // other stream the screens are from now on dirty there
  template <class Q> int ring_write(Q &q, void *s, void *atm_stream, bool overlap) {
    if (s != atm_stream) { screens_dirty_main = true; return 0; }
    if (overlap && ev_frame_prev) {
      if (need_prev) { int rc = q.wait(s, ev_frame_prev); if (rc) return rc; need_prev = false; }
    } else if (frame_wait_pending) {
      int rc = q.wait(s, ev_frame_cur);
      if (rc) return rc;
      frame_wait_pending = false; need_prev = false;
    }
    return 0;
  }
  // the screens were written on the caller's stream (reset, adopted reset, set_screen): the next prefetch waits at once
  void screens_written() { screens_dirty_main = true; }

  // a prefetch begins behind the frame launched on `stream`: the readers are marked (reuse_mark: by that frame's own
  // closing event, if nothing was launched since), the extrusion stream forks into a capture, and it waits for the
  // readers right away if the screens were last written on the caller's stream -- else its first ring write will
  // (the stencil gather and the product of the first round only READ the screens, like the frame kernel just launched:
  // they run beside it; writes made on the caller's stream are ordered before this point of THAT stream only)
  template <class Q> int prefetch_begin(Q &q, void *stream, void *atm_stream, void *ev_frame, void *ev_fork, bool reuse_mark,
                                        bool capturing) {
    if (!(reuse_mark && frame_marked)) {
      int rc = q.record(ev_frame, stream);
      if (rc) return rc;
      ev_frame_cur = ev_frame;
    }
    side_joined = false;
    if (capturing) {
      if (!fork_recorded) { int rc = q.record(ev_fork, stream); if (rc) return rc; fork_recorded = true; }
      int rc = q.wait(atm_stream, ev_fork);
      if (rc) return rc;
    }
    if (screens_dirty_main) {
      int rc = q.wait(atm_stream, ev_frame_cur);
      if (rc) return rc;
      frame_wait_pending = false;
    } else {
      frame_wait_pending = true;
    }
    return 0;
  }
  // a prefetch ends: ev_moved stands behind the readers even if nothing was extruded, and is recorded unless the
  // move's last launch carried it; the move of [b, b + n) is pending, the screens are clean on the caller's stream
  template <class Q> int prefetch_end(Q &q, void *atm_stream, void *ev_moved, bool carried, const void *screens, int b, int n) {
    if (frame_wait_pending) {
      int rc = q.wait(atm_stream, ev_frame_cur);
      if (rc) return rc;
      frame_wait_pending = false;
    }
    screens_dirty_main = false;
    if (!carried) { int rc = q.record(ev_moved, atm_stream); if (rc) return rc; }
    premoved = true; pre_screens = screens; pre_b = b; pre_n = n;
    return 0;
  }
  // is the move of exactly this range already done?  Then it is consumed
  bool take_move(const void *screens, int b, int n) {
    if (!move_is(screens, b, n)) return false;
    premoved = false;
    return true;
  }
  // a reset of [b, b + n) against the pending move of these screens: one that covers it drops it
  MoveOverlap reset_range(const void *screens, int b, int n) {
    if (!move_pending_on(screens)) return MOVE_NONE;
    const bool covers = b <= pre_b && b + n >= pre_b + pre_n;
    const bool disjoint = b + n <= pre_b || b >= pre_b + pre_n;
    if (covers) premoved = false;
    return covers ? MOVE_COVERED : disjoint ? MOVE_DISJOINT : MOVE_OVERLAPS;
  }

  // a frame was launched with this closing event; side (a plain frame with the prefetch on): the event is the readers'
  // mark, the side streams have work of their own again, and the PSF stream is behind the frame
  template <class Q> int frame_launched(Q &q, bool side, void *psf_stream, void *ev_done) {
    frame_marked = false;
    if (!side) return 0;
    ev_frame_cur = ev_done; frame_marked = true;
    side_joined = false;
    return q.wait(psf_stream, ev_done);
  }
  // that frame's PSF finish was launched on the PSF stream (a captured dispatch carries no event: recorded here)
  template <class Q> int psf_finish_launched(Q &q, bool capturing, void *ev_psf, void *psf_stream) {
    if (capturing) { int rc = q.record(ev_psf, psf_stream); if (rc) return rc; }
    psf_side = true;
    return 0;
  }

  // a pipelined prefetch begins: two frames in flight, the move's first ring write picks which one it is behind
  void pipe_prefetch_begin(void *ev_older, void *ev_newest) {
    side_joined = false;
    ev_frame_prev = ev_older; need_prev = true;
    ev_frame_cur = ev_newest; frame_wait_pending = true;
  }
  // its move is over; copy_follows (a ring did not move: all origins are copied into the older frame's snapshot):
  // that copy is behind the older frame if no ring write was.  No older frame is known past this point
  template <class Q> int pipe_move_end(Q &q, void *atm_stream, bool copy_follows) {
    int rc = 0;
    if (copy_follows && need_prev && frame_wait_pending) rc = q.wait(atm_stream, ev_frame_prev);
    ev_frame_prev = nullptr; need_prev = false; frame_wait_pending = false;
    return rc;
  }
  // the pipelined frame takes the pending move: its stream is behind it, whatever the caller's stream has joined
  template <class Q> int frame_takes_move(Q &q, void *frame_stream, void *ev_moved) {
    int rc = q.wait(frame_stream, ev_moved);
    if (rc) return rc;
    premoved = false;
    return 0;
  }
  // the pipeline adopts the plain frame that started it: its PSF finish is the pipeline's to wait for; its mark
  void *pipe_adopts_plain_frame() { psf_side = false; return ev_frame_cur; }

  // ---- the step as a HIP graph
  // work that plain calls left on the side streams is waited for OUTSIDE the graph, once
  template <class Q> int graph_join_outside(Q &q, void *stream, void *ev_moved, void *ev_psf) {
    if (side_joined) return 0;
    int rc = q.wait(stream, ev_moved);
    if (rc) return rc;
    if (psf_side) { rc = q.wait(stream, ev_psf); if (rc) return rc; }
    side_joined = true;
    return 0;
  }
  void capture_begin() { fork_recorded = false; }
  // where the extrusion stream forks from the caller's, in front of the frame kernel
  template <class Q> int capture_fork(Q &q, void *ev_fork, void *stream) {
    int rc = q.record(ev_fork, stream);
    if (rc) return rc;
    fork_recorded = true;
    return 0;
  }
  // the side streams join the caller's stream again at the end of a captured body
  template <class Q> int capture_join(Q &q, void *stream, void *ev_psf, void *ev_moved) {
    if (psf_side) { int rc = q.wait(stream, ev_psf); if (rc) return rc; }
    if (premoved) { int rc = q.wait(stream, ev_moved); if (rc) return rc; }
    side_joined = true;
    return 0;
  }
  // a captured step was replayed: what its body left behind when it was recorded
  void replayed(bool prefetch) {
    if (prefetch) {
      premoved = true; psf_side = true; side_joined = true;
      frame_marked = true; frame_wait_pending = false; screens_dirty_main = false;
    } else {
      frame_marked = false; screens_dirty_main = true;
    }
  }
};
