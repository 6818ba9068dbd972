"""The launch sequence of a move or a reset of the atmosphere (csrc/aomarl_move_plan_host.h), CPU side: the stand-alone
program around the host-only plan under the address and undefined-behaviour sanitizers -- its invariants over every
combination of layers, classes, shifts, "extrude_unfused" and the line-length limits -- and the plan itself against the
pinned table of what the launch code it replaced decided (ExtrudeRun::step, run_plan, move_atmos_now, reset_rounds_plan,
reset_parts, step_plan_uniform)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ao_marl_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "move_plans.txt")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("move_plan") / "move_plan_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(CSRC, "move_plan_host_check.cpp")])
    out = subprocess.run([exe, "--table"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def pinned():
    with open(GOLDEN) as fh:
        return fh.read().splitlines()


def section(lines, title):
    """the lines of one case, without its '# ...' header"""
    start = [i for i, ln in enumerate(lines) if ln.startswith("# %s:" % title)]
    assert len(start) == 1, title
    out = []
    for ln in lines[start[0] + 1:]:
        if ln.startswith("# "):
            break
        out.append(ln)
    return out


def launches(lines):
    """(part, round, kind) of every launch record (part: "" for a move, "p<k>" for a reset)"""
    recs = [ln.split() for ln in lines if ln.startswith("  ")]
    return [tuple(t[:3]) if t[0].startswith("p") else ("",) + tuple(t[:2]) for t in recs]


def test_host_check_builds_and_passes(table):
    """rounds: (25 + 2 x 25^2 + 4 x 25^3) shifts and class assignments x 3 line lengths x "extrude_unfused" on / off;
    then the margin predicate, the groups of 4^5 batches, the reset partition of 9 sizes x 4 stream counts x 8 x 2"""
    rounds = (25 + 2 * 25 ** 2 + 4 * 25 ** 3) * 3 * 2
    assert table[-1] == "move_plan_host_check: ok (%d combinations)" % (rounds + 4 * 4 * 5 * 125 + 1024 + 9 * 4 * 8 * 2)


def test_plan_is_the_pinned_table(table, pinned):
    """one line per launch record (kind, sub-round, reference layer, Z parity, is_write, may_ride, the next round of a
    fused scatter + gather), per group (range, shift, rounds, small, overlap, complete) and per partition: recorded from
    the launch code the plan replaced, line for line"""
    got = table[:-1]
    assert len(got) == len(pinned)
    bad = [i for i, (a, b) in enumerate(zip(got, pinned)) if a != b]
    assert not bad, "line %d: %r, pinned %r" % (bad[0] + 1, got[bad[0]], pinned[bad[0]])


def test_the_named_cases_read_off_the_pinned_table(pinned):
    # three layers of one class finishing at rounds 1, 3 and 2: one gather, then product | scatter + gather; the rounds
    # thin out 3 -> 2 -> 1 operations, the parity alternates, the last scatter is plain and may ride
    thin = section(pinned, "move thin3")
    assert [k for _, _, k in launches(thin)] == ["GATHER", "PRODUCT", "SCATTER_GATHER", "PRODUCT", "SCATTER_GATHER", "PRODUCT", "SCATTER"]
    assert "ops 0:1:0 1:1:0 2:-1:0 next 2 idx -1 0 1 -1 -1 -1 -1 -1 dir 1 -2 0" in thin[6]      # layer 0 is done, layer 2 turns to y
    assert "ops 1:1:0 2:-2:0 next 1 idx 0 -1 -1" in thin[8] and " par 1 " in thin[8]
    assert thin[10].split()[:2] == ["r2", "SCATTER"] and " par 0 w 1 ride 1 ops 1:2:0" in thin[10]
    # "extrude_unfused", a stencil or a line too long for k_extrude_sg: three launches per round, one parity
    for name in ("thin3_unfused", "thin3_long_stencil", "thin3_long_line"):
        sec = section(pinned, "move " + name)
        assert [k for _, _, k in launches(sec)] == ["GATHER", "PRODUCT", "SCATTER"] * 3 and not [ln for ln in sec if " par 1 " in ln]
    # two classes: nothing fuses while both have work; the last round is class 0 alone, so nothing may ride
    two = section(pinned, "move two_class")
    assert [(r, k) for _, r, k in launches(two)] == [("r0", k) for k in ["GATHER", "PRODUCT", "SCATTER"] * 2] + \
        [("r1", "GATHER"), ("r1", "PRODUCT"), ("r1", "SCATTER_GATHER"), ("r2", "PRODUCT"), ("r2", "SCATTER")]
    assert not [ln for ln in two if " ride 1" in ln]
    assert section(pinned, "move two_class_last_rides")[-4].endswith("SCATTER ref 1 par 0 w 1 ride 1 ops 1:1:0")
    # a y shift behind an x shift: dir 1 once, then dir -2 twice
    yx = section(pinned, "move y_behind_x")
    assert [ln.split("ops ")[1].split()[0] for ln in yx if " PRODUCT " in ln] == ["0:1:0", "0:-2:0", "0:-2:0"]
    # a batch of three groups: the middle one does not move and launches nothing, the last takes two lines in layer 1
    three = section(pinned, "move three_groups")
    assert three[0] == "uniform 0"
    groups = [ln for ln in three if ln.startswith("group")]
    assert groups == ["group 0 2 shift 1:0 0:1 0:0 rounds 1 small 0 overlap 0 complete 0",
                      "group 2 1 shift 0:0 0:0 0:0 rounds 0 small 0 overlap 0 complete 0",
                      "group 3 3 shift 0:0 2:0 1:-1 rounds 2 small 0 overlap 0 complete 0"]
    assert three[three.index(groups[1]) + 1] == groups[2] and "complete 0" in three
    # the small move: one launch per moving group, it writes and may ride
    small = section(pinned, "move three_groups_small")
    assert [ln.split()[:9] for ln in small if ln.startswith("  ")] == [["r0", "MOVE_SMALL", "ref", "-1", "par", "0", "w", "1", "ride"]] * 2
    assert small[-4].endswith("shift 0:0 2:0 1:-1 0:0 0:0 0:0 0:0 0:0")
    # beside the older frame in flight only inside the margins, group by group
    assert [ln.split("overlap ")[1][0] for ln in section(pinned, "move older_two_groups") if ln.startswith("group")] == ["1", "0"]
    # resets of two layers (dims 4 and 6, a class each): 12 rounds; two sub-rounds while both grow (8 rounds), then layer 1
    # alone fuses; transposed: dir +-2 with tflag 1, untransposed: dir +-1 with tflag 0
    tr, un = section(pinned, "reset transposed"), section(pinned, "reset untransposed")
    assert tr[0] == un[0] == "rounds 12 parts 1: 0 4 pick 0"
    assert len(launches(tr)) == len(launches(un)) == 8 * 6 + 3 + 3 * 2
    assert tr[1].endswith("ops 0:2:1") and tr[4].endswith("ops 1:-2:1") and un[1].endswith("ops 0:1:0") and un[4].endswith("ops 1:-1:0")
    assert [k for _, r, k in launches(tr) if r == "r9"] == ["PRODUCT", "SCATTER_GATHER"]
    # the partition: 33 environments in parts of 16 and 17, round by round and part by part
    parts = section(pinned, "reset two_parts")
    assert parts[0] == "rounds 12 parts 2: 3 16 pick 0 19 17 pick 0"
    assert [w for w, r, _ in launches(parts) if r == "r0"] == ["p0"] * 6 + ["p1"] * 6
    # the prefetched reset two rounds at a time: the whole range with a part's split where it divides, else the parts
    whole = section(pinned, "reset prefetched_whole_by_two")
    assert whole[0] == "rounds 12 parts 1: 0 32 pick 16" and whole.count("advance 2") == 6
    assert [r for _, r, _ in launches(whole[whole.index("advance 2", 2):])][:12] == ["r2"] * 6 + ["r3"] * 6
    assert section(pinned, "reset prefetched_parts_by_two")[0] == "rounds 12 parts 2: 0 16 pick 0 16 17 pick 0"
    assert not [ln for ln in section(pinned, "reset prefetched_unfused_by_five") if "SCATTER_GATHER" in ln]
