"""Which chain aomarl_env_step runs (csrc/aomarl_step_plan_host.h), CPU side: the stand-alone program around the host-only
plan under the address and undefined-behaviour sanitizers -- its invariants over every combination of the facts -- and the
plan itself against the pinned table of what the four predicates it replaced decided."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ao_marl_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "step_plans.txt")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_plan") / "step_plan_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(CSRC, "step_plan_host_check.cpp")])
    out = subprocess.run([exe, "--table"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def test_host_check_builds_and_passes(table):
    """every one of the 2^24 combinations of the boolean facts keeps the invariants the header promises"""
    assert table[-1] == "step_plan_host_check: ok (%d combinations)" % 2 ** 24


def test_plan_is_the_pinned_table(table):
    """head, sense and tail for all 4096 combinations of the facts that decide them, the route for all 512 of what it
    depends on (the pipeline's own conditions all holding / each one alone failing): recorded from the predicates the plan
    replaced (small_chain_ok, env_step_fusable, env_step_shortcut, pipe_eligible), line for line"""
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    assert len(want) == 1 + 4096 + 1 + 512
    got = table[:-1]
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, "line %d: %r, pinned %r" % (bad[0] + 1, got[bad[0]], want[bad[0]])
    # the cases the issue names, read off the pinned table itself
    rows = dict(line.split(" ", 1) for line in want[1:4097])
    #            unfused one_tt no_other defer mgain env_gain small_opt fits cmat shortcut_opt s2m denoiser
    assert rows["010100111111"] == "HEAD_SMALL SENSE_DENOISER TAIL_FUSED"      # a denoiser on a small system
    assert rows["010100111110"] == "HEAD_SMALL SENSE_FRAME TAIL_SMALL"         # small wins over the shortcut
    assert rows["010100011110"] == "HEAD_FUSED SENSE_FRAME TAIL_SHORTCUT"
    assert rows["010110111110"] == "HEAD_STAGES SENSE_FRAME TAIL_STAGES"       # modal gains
    assert rows["110100111110"] == "HEAD_STAGES SENSE_FRAME TAIL_STAGES"       # UNFUSED
