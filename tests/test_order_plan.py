"""How a context's side streams are ordered against the caller's stream (csrc/aomarl_order_host.h), CPU side: the
stand-alone program around the ledger under the address and undefined-behaviour sanitizers -- its invariants over every
reachable state -- and every edge it prints against the rules as their call sites spelled them before there was a ledger.
That expectation is written out here, in Python, function by function from those sites as they stood (psf_wait_pending,
atmos_wait_pending, first_write_wait and ExtrudeRun::launch, prefetch_atmos_impl, aomarl_move_atmos, reset_prologue,
aomarl_target_image, the tail of frame_fused_impl, next_part_one_sense, pipe_launch_frame, pipe_prefetch,
env_step_pipelined, fw_ev_rewind and the graph path of aomarl_env_step), on a context with the fields they used, with a
breadth-first walk of its own over the same calls: it reads nothing back from the header under test.  One thing is the
header's alone: `outstanding` (a prefetched move or a pipelined prefetch is under way), a query no call site had."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ao_marl_amd", "csrc")

STREAMS = ("main", "atm", "other")
RANGES = ((0, 4), (0, 2), (2, 2), (1, 2))           # (b, n): the batch of 4, its halves, its middle
NENV = 4

FIELDS = ("premoved", "pre_screens", "pre_b", "pre_n", "frame_wait_pending", "screens_dirty_main", "side_joined",
          "fork_recorded", "frame_marked", "ev_frame_cur", "ev_frame_prev", "need_prev", "psf_side", "made")


class Ctx:
    """the fourteen loose fields of aomarl_ctx (snap_target, an argument passed through the context, orders nothing and is
    not walked), `made`: side_stream() has run, and the handles it creates (null before)"""
    __slots__ = FIELDS + ("ops",)

    def __init__(self, state):
        for k, v in zip(FIELDS, state):
            setattr(self, k, v)
        self.ops = []

    def state(self):
        return tuple(getattr(self, k) for k in FIELDS)

    def handle(self, name):
        return name if self.made else None

    atm_stream = property(lambda self: self.handle("atm"))
    psf_stream = property(lambda self: self.handle("psf"))
    ev_frame = property(lambda self: self.handle("ev_frame"))
    ev_moved = property(lambda self: self.handle("ev_moved"))
    ev_psf = property(lambda self: self.handle("ev_psf"))
    ev_fork = property(lambda self: self.handle("ev_fork"))

    def wait(self, stream, event):                   # hipStreamWaitEvent(stream, event, 0)
        self.ops.append("wait(%s,%s)" % (stream or "-", event or "-"))

    def record(self, event, stream):                 # hipEventRecord(event, stream)
        self.ops.append("record(%s,%s)" % (event or "-", stream or "-"))


FRESH = (False, None, 0, 0, False, True, False, False, False, None, None, False, False, False)


# ---- aomarl_capi_atmos.hip as it stood
def side_stream(c):
    if not c.made:
        c.made = True
        c.ev_frame_cur = c.ev_frame


def psf_wait_pending(c, stream):
    if c.psf_side and not c.side_joined:
        c.wait(stream, c.ev_psf)
    c.psf_side = False


def atmos_wait_pending(c, stream):
    if c.premoved and not c.side_joined:
        c.wait(stream, c.ev_moved)


def first_write_wait(c, s, overlap):
    if s != c.atm_stream:
        return
    if overlap and c.ev_frame_prev:
        if c.need_prev:
            c.wait(s, c.ev_frame_prev)
            c.need_prev = False
    elif c.frame_wait_pending:
        c.wait(s, c.ev_frame_cur)
        c.frame_wait_pending = False
        c.need_prev = False


def extrude_launch_write(c, s, overlap):
    """ExtrudeRun::launch, `if (L.is_write && ordered)`"""
    first_write_wait(c, s, overlap)
    if s != c.atm_stream:
        c.screens_dirty_main = True


def prefetch_atmos_impl_before_move(c, stream, frame_marked, capturing):
    side_stream(c)
    if not frame_marked:
        c.record(c.ev_frame, stream)
        c.ev_frame_cur = c.ev_frame
    c.side_joined = False
    if capturing:
        if not c.fork_recorded:
            c.record(c.ev_fork, stream)
            c.fork_recorded = True
        c.wait(c.atm_stream, c.ev_fork)
    if c.screens_dirty_main:
        c.wait(c.atm_stream, c.ev_frame_cur)
        c.frame_wait_pending = False
    else:
        c.frame_wait_pending = True


def prefetch_atmos_impl_behind_move(c, rode, screens, b, n):
    """also the end of pipe_prefetch behind its own tear-down (frame_wait_pending is false there), with
    rode = done.rode && complete"""
    if c.frame_wait_pending:
        c.wait(c.atm_stream, c.ev_frame_cur)
        c.frame_wait_pending = False
    c.screens_dirty_main = False
    if not rode:
        c.record(c.ev_moved, c.atm_stream)
    c.premoved = True
    c.pre_screens, c.pre_b, c.pre_n = screens, b, n


def move_atmos_consumes(c, screens, b, n):
    """aomarl_move_atmos behind its atmos_wait_pending"""
    if c.premoved:
        if c.pre_screens == screens and c.pre_b == b and c.pre_n == n:
            c.premoved = False
            return "taken"
    return "not"


def reset_prologue(c, screens, b, n):
    if c.premoved and c.pre_screens == screens:
        covers = b <= c.pre_b and b + n >= c.pre_b + c.pre_n
        disjoint = b + n <= c.pre_b or b >= c.pre_b + c.pre_n
        if covers:
            c.premoved = False
            return "covered"
        if not disjoint:                             # the ranges of the fail() text
            return "overlaps [%d, %d)" % (c.pre_b, c.pre_b + c.pre_n)
        return "disjoint"
    return "none"


# ---- aomarl_capi_composites.hip
def frame_fused_tail(c, side, ev_done):
    """frame_fused_impl behind the launch; side: slot < 0 with "prefetch_atmos" on (side_stream() ran in front)"""
    c.frame_marked = False
    if side:
        c.ev_frame_cur = ev_done
        c.frame_marked = True
        c.side_joined = False
        c.wait(c.psf_stream, ev_done)


def frame_fused_behind_finish(c, capturing):
    if capturing:
        c.record(c.ev_psf, c.psf_stream)
    c.psf_side = True


def next_part_one_fork(c, stream):
    side_stream(c)
    c.record(c.ev_fork, stream)
    c.fork_recorded = True


# ---- aomarl_capi_step.hip
def pipe_launch_frame_takes(c):
    c.wait("fstream", c.ev_moved)
    c.premoved = False


def pipe_prefetch_setup(c, older, newest):
    c.side_joined = False
    c.ev_frame_prev, c.need_prev = older, True
    c.ev_frame_cur, c.frame_wait_pending = newest, True


def pipe_prefetch_teardown(c, rc_ok_and_incomplete):
    if rc_ok_and_incomplete and c.need_prev and c.frame_wait_pending:
        c.wait(c.atm_stream, c.ev_frame_prev)
    c.ev_frame_prev, c.need_prev, c.frame_wait_pending = None, False, False


def pipelined_first_step_adopts(c):
    ev = c.ev_frame_cur                              # P.ev_done_cur[0] = c->ev_frame_cur
    c.psf_side = False
    return ev or "-"


def graph_join_outside(c, s):
    side_stream(c)
    if not c.side_joined:
        c.wait(s, c.ev_moved)
        if c.psf_side:
            c.wait(s, c.ev_psf)
        c.side_joined = True


def graph_replayed(c, pf):
    if pf:
        c.premoved = c.psf_side = c.side_joined = True
        c.frame_marked = True
        c.frame_wait_pending = c.screens_dirty_main = False
    else:
        c.frame_marked = False
        c.screens_dirty_main = True


def graph_capture_join(c, s):
    if c.psf_side:
        c.wait(s, c.ev_psf)
    if c.premoved:
        c.wait(s, c.ev_moved)
    c.side_joined = True                             # `if (pf) c->side_joined = true` behind the capture


def queries(c):
    on = lambda scr: c.premoved and c.pre_screens == scr                                   # aomarl_target_image
    whole = on("A") and c.pre_b == 0 and c.pre_n == NENV                                   # pipe_launch_frame, the graph's steady state
    steady = not (not c.premoved or not c.psf_side)                                        # env_step_pipelined
    return "pending=%d on_A=%d on_B=%d whole_A=%d older=%d steady=%d outstanding=%d held=%s,%s" % (
        c.premoved, on("A"), on("B"), whole, c.ev_frame_prev is not None, steady,
        c.premoved or c.ev_frame_prev is not None, c.ev_frame_cur or "-", c.ev_frame_prev or "-")       # held: fw_ev_rewind


def fmt(state):
    v = dict(zip(FIELDS, state))
    return "pm=%d scr=%s b=%d n=%d fwp=%d dirty=%d joined=%d fork=%d marked=%d cur=%s prev=%s need=%d psf=%d made=%d" % (
        v["premoved"], v["pre_screens"] or "-", v["pre_b"], v["pre_n"], v["frame_wait_pending"], v["screens_dirty_main"],
        v["side_joined"], v["fork_recorded"], v["frame_marked"], v["ev_frame_cur"] or "-", v["ev_frame_prev"] or "-",
        v["need_prev"], v["psf_side"], v["made"])


def calls(state):
    """every call of the walk from this state, under the condition its call site put in front of it: (text, function
    of a context returning the result or None)"""
    f = dict(zip(FIELDS, state))
    made, premoved = f["made"], f["premoved"]
    whole = premoved and f["pre_screens"] == "A" and f["pre_b"] == 0 and f["pre_n"] == NENV
    out = []
    for s in STREAMS:
        if s == "atm" and not made:
            continue
        out.append(("psf_join(%s)" % s, lambda c, s=s: psf_wait_pending(c, s)))
        out.append(("move_join(%s)" % s, lambda c, s=s: atmos_wait_pending(c, s)))
        for ov in (0, 1):
            out.append(("ring_write(%s,%d)" % (s, ov), lambda c, s=s, ov=ov: extrude_launch_write(c, s, bool(ov))))
    out.append(("screens_written()", lambda c: setattr(c, "screens_dirty_main", True)))      # aomarl_reset, _reset_adopt, _set_screen
    if not premoved:                                 # "prefetch_atmos: a prefetched frame is already pending"
        for reuse in (0, 1):                         # aomarl_prefetch_atmos passed false, next_part_one_sense c->frame_marked
            for cap in (0, 1):
                out.append(("prefetch_begin(main,%d,%d)" % (reuse, cap), lambda c, reuse=reuse, cap=cap:
                            prefetch_atmos_impl_before_move(c, "main", bool(reuse) and c.frame_marked, bool(cap))))
    if made and not premoved:
        for rode in (0, 1):
            for b, n in RANGES[:2]:
                out.append(("prefetch_end(%d,A,%d,%d)" % (rode, b, n), lambda c, rode=rode, b=b, n=n:
                            prefetch_atmos_impl_behind_move(c, bool(rode), "A", b, n)))
    for scr in ("A", "B"):
        for b, n in RANGES:
            out.append(("take_move(%s,%d,%d)" % (scr, b, n), lambda c, scr=scr, b=b, n=n: move_atmos_consumes(c, scr, b, n)))
            out.append(("reset_range(%s,%d,%d)" % (scr, b, n), lambda c, scr=scr, b=b, n=n: reset_prologue(c, scr, b, n)))
    out.append(("queries()", queries))
    out.append(("frame_launched(0,-)", lambda c: frame_fused_tail(c, False, None)))
    for ev in ("ev_frame", "ev_timed"):
        out.append(("frame_launched(1,%s)" % ev, lambda c, ev=ev: (side_stream(c), frame_fused_tail(c, True, ev))[0]))
    if made:
        for cap in (0, 1):
            out.append(("psf_finish_launched(%d)" % cap, lambda c, cap=cap: frame_fused_behind_finish(c, bool(cap))))
    out.append(("capture_fork(main)", lambda c: next_part_one_fork(c, "main")))
    if made and not premoved:                        # "frame pipeline: a prefetched frame is already pending"
        for older, newest in (("ev_done0", "ev_done1"), ("ev_done1", "ev_done0"), ("mark", "ev_done1")):
            out.append(("pipe_prefetch_begin(%s,%s)" % (older, newest), lambda c, older=older, newest=newest:
                        pipe_prefetch_setup(c, c.ev_frame_cur if older == "mark" else older, newest)))
    if made:
        for copy in (0, 1):
            out.append(("pipe_move_end(%d)" % copy, lambda c, copy=copy: pipe_prefetch_teardown(c, bool(copy))))
    if whole:                                        # "frame pipeline: no prefetched atmosphere frame of the whole batch is pending"
        out.append(("frame_takes_move()", pipe_launch_frame_takes))
    if premoved and f["psf_side"]:
        out.append(("pipe_adopts_plain_frame()", pipelined_first_step_adopts))
    if whole:                                        # `steady` with the prefetch on
        out.append(("graph_join_outside(main)", lambda c: graph_join_outside(c, "main")))
        out.append(("replayed(1)", lambda c: graph_replayed(c, True)))
    if not premoved:                                 # `steady` with the prefetch off
        out.append(("replayed(0)", lambda c: graph_replayed(c, False)))
    out.append(("capture_begin()", lambda c: setattr(c, "fork_recorded", False)))
    if made:
        out.append(("capture_join(main)", lambda c: graph_capture_join(c, "main")))
    return out


def walk():
    seen = {FRESH}
    todo = [FRESH]
    edges = []
    for state in todo:                               # (grows while it is walked: breadth first)
        head = fmt(state)
        for text, fn in calls(state):
            c = Ctx(state)
            result = fn(c)
            for op in c.ops:
                assert "-" not in op, (head, text, op)            # no operation on a null handle
            to = c.state()
            if to not in seen:
                seen.add(to)
                todo.append(to)
            edges.append("%s | %s | %s | %s | %s" % (head, text, " ".join(c.ops) or "-", result or "-", fmt(to)))
    return seen, edges


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("order_plan") / "order_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(CSRC, "order_host_check.cpp")])
    out = subprocess.run([exe, "--table"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    return lines[-1], lines[:-1], [line.split(" | ") for line in lines[:-1]]      # the verdict, the edges, their five parts


@pytest.fixture(scope="module")
def before():
    return walk()


def test_host_check_builds_and_passes(table):
    """the invariants hold on every edge, and the program printed as many edges as it counted"""
    verdict, lines, parts = table
    m = re.fullmatch(r"order_host_check: ok \((\d+) states, (\d+) edges\)", verdict)
    assert m and int(m.group(2)) == len(lines)
    assert int(m.group(1)) == len({p[0] for p in parts} | {p[4] for p in parts})


def test_every_edge_is_what_the_call_sites_did(table, before):
    """the same states, the same edges, the same operations and the same successor on each; and this walk reaches no fewer
    states than the program says it did, so neither side passes by exploring less"""
    seen, edges = before
    verdict, lines, parts = table
    nstates = int(re.search(r"\((\d+) states", verdict).group(1))
    assert len(seen) >= nstates
    assert len(edges) == len(lines)
    ours, theirs = set(edges), set(lines)
    assert len(ours) == len(edges)                   # (an edge is its state and its call: none twice)
    assert sorted(ours - theirs)[:5] == [] and sorted(theirs - ours)[:5] == []
    assert {fmt(s) for s in seen} == {p[0] for p in parts}


def test_the_walk_meets_every_rule(before):
    """each call occurs, with and without operations where it has any to issue; every wait that may be skipped is skipped
    somewhere and issued somewhere"""
    _, edges = before
    with_ops, without = set(), set()
    results = set()
    for e in edges:
        p = e.split(" | ")
        name = p[1].split("(")[0]
        (without if p[2] == "-" else with_ops).add(name)
        if name in ("take_move", "reset_range"):
            results.add(p[3].split(" ")[0])
    assert with_ops | without == {"psf_join", "move_join", "ring_write", "screens_written", "prefetch_begin", "prefetch_end",
                                  "take_move", "reset_range", "queries", "frame_launched", "psf_finish_launched",
                                  "capture_fork", "pipe_prefetch_begin", "pipe_move_end", "frame_takes_move",
                                  "pipe_adopts_plain_frame", "graph_join_outside", "replayed", "capture_begin", "capture_join"}
    assert {"psf_join", "move_join", "ring_write", "prefetch_end", "pipe_move_end", "graph_join_outside", "capture_join",
            "psf_finish_launched", "frame_launched"} <= with_ops & without
    assert results == {"taken", "not", "none", "covered", "disjoint", "overlaps"}


def test_field_names_live_in_the_header_alone():
    """the done-criterion: outside the ledger, its host check and this test, no file of csrc names one of the fourteen fields"""
    names = re.compile(r"\b(premoved|pre_screens|pre_b|pre_n|frame_wait_pending|screens_dirty_main|side_joined|fork_recorded|"
                       r"frame_marked|ev_frame_cur|ev_frame_prev|need_prev|psf_side|snap_target)\b")
    for fn in sorted(os.listdir(CSRC)):
        if fn in ("aomarl_order_host.h", "order_host_check.cpp") or not fn.endswith((".hip", ".h", ".cpp")):
            continue
        with open(os.path.join(CSRC, fn)) as fh:
            assert not names.search(fh.read()), fn
