"""Which instantiation of the staged Shack-Hartmann and science-target kernels a call gets, its grid and its dynamic LDS
(csrc/aomarl_stage_plan_host.h), CPU side: the stand-alone program around the host-only plan under the address and
undefined-behaviour sanitizers -- its invariants over the whole query space -- and every plan it prints against what
aomarl_comp_image and target_psf_impl decided before there was a plan.  That expectation is written out here, in Python,
from those two functions as they stood (the refusals and the 24-way ladder of the one, the three branches and their
byte counts of the other): it reads nothing back from the header under test."""
import itertools
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ao_marl_amd", "csrc")

LAYERS, NVALID, NENV = (1, 3), (1, 5, 1264), (1, 7, 4096)
HW, NPSF, PUPDIAM = (4, 8, 16), (64, 4096, 4098), (48, 320)

# the strings aomarl_comp_image passed to fail(), in the order it tested them
REFUSALS = (
    "comp_image: FROM_PHASE_BUFFER needs st->wfs_phase",
    "comp_image: fused raytrace needs integer layer offsets; use raytrace_wfs + FROM_PHASE_BUFFER",
    "comp_image: WRITE_BINCUBE needs st->bincube",
    "comp_image: nothing to produce (neither bincube nor slopes)",
)


def tf(b):
    return "true" if b else "false"


def comp_image_before(from_buf, noise, cube, cog, na, nd, force_generic_spot, production_layout, wfs_phase, bincube,
                      wfs_all_int, nlayers, nvalid, n):
    """aomarl_comp_image behind its range checks, line by line: the refusal's text, or the launch"""
    if from_buf and not wfs_phase:
        return "refused: " + REFUSALS[0]
    if not from_buf and not wfs_all_int:
        return "refused: " + REFUSALS[1]
    if cube and not bincube:
        return "refused: " + REFUSALS[2]
    if not cube and not cog:
        return "refused: " + REFUSALS[3]
    gx = (16384 + 4 * n - 1) // (4 * n)
    gx = max(1, min(gx, (nvalid + 3) // 4))
    grid = " grid=%dx%d block=256" % (gx, n)
    fast_ok = not from_buf and not na and not nd and not force_generic_spot and production_layout
    if fast_ok:
        return "k_wfs_spot_fast<%d, %s, %s>(cog=%d)" % (1 if nlayers == 1 else 3, tf(noise), tf(cube), cog) + grid
    return "k_wfs_spot<%s, %s, %s>(no_atmos=%d, no_dms=%d, cog=%d)" % (tf(from_buf), tf(noise), tf(cube), na, nd, cog) + grid


def target_psf_before(hw, npsf, pupdiam, nlayers, from_buf, production_layout, force_valu_target, force_generic_target, nblk, n):
    """target_psf_impl's three branches, each with the byte count it spelled inline (4: sizeof(float))"""
    tw = 4 * 2 * npsf if npsf <= 4096 else 0
    grid = " grid=%dx%d block=256" % (nblk, n)
    mfma_finish = " nblk=%d | k_target_finish_mfma grid=%d block=256" % (nblk, n)
    if hw == 8 and not force_valu_target and not force_generic_target and not from_buf and production_layout:
        smm = 4 * (4 * 16 * 65 + 4 * 2 * 256) + tw
        return "k_target_rows_fast<%d>" % (1 if nlayers == 1 else 3) + grid + " lds=%d" % smm + mfma_finish
    if hw == 8 and not force_valu_target:
        smm = 4 * (2 * 16 * 65 + 4 * 2 * 256) + tw
        return "k_target_rows_mfma<%s>" % tf(from_buf) + grid + " lds=%d" % smm + mfma_finish
    W = 2 * hw
    RB = 256 // W
    sm = 4 * (2 * RB * 64 + 3 * 256) + tw           # TGT_XC was 64
    return "k_target_rows<%s>" % tf(from_buf) + grid + " lds=%d nblk=%d | k_target_finish grid=%d block=256" % (sm, nblk, n)


def spot_queries():
    """the program's order: the eleven booleans as bits 0 .. 10 of a counter, then nlayers, nvalid, n"""
    for b in range(1 << 11):
        bits = [(b >> k) & 1 for k in range(11)]
        for nl, nvalid, n in itertools.product(LAYERS, NVALID, NENV):
            yield bits, nl, nvalid, n


def target_queries():
    for b in range(1 << 4):
        bits = [(b >> k) & 1 for k in range(4)]
        for hw, npsf, pd, nl, n in itertools.product(HW, NPSF, PUPDIAM, LAYERS, NENV):
            rb = 256 // (2 * hw)                     # work_layout: nblk = ceil(pupdiam / RB)
            yield bits, hw, npsf, pd, nl, (pd + rb - 1) // rb, n


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_plan") / "stage_plan_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(CSRC, "stage_plan_host_check.cpp")])
    out = subprocess.run([exe, "--table"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


NSPOT = (1 << 11) * len(LAYERS) * len(NVALID) * len(NENV)
NTARGET = (1 << 4) * len(HW) * len(NPSF) * len(PUPDIAM) * len(LAYERS) * len(NENV)


def test_host_check_builds_and_passes(table):
    """the whole query space of both planners keeps what a launch needs (grid bounds, LDS carve-up, stripes over the pupil)"""
    assert table[-1] == "stage_plan_host_check: ok (%d + %d queries)" % (NSPOT, NTARGET)
    assert len(table) == NSPOT + NTARGET + 1


def test_spot_plans_are_what_comp_image_decided(table):
    """every line of plan_spot: the facts it was asked with, then the refusal or the launch of the ladder it replaced"""
    names = ("from_buf", "noise", "cube", "cog", "no_atmos", "no_dms", "force_generic_spot", "production_layout", "wfs_phase",
             "bincube", "wfs_all_int")
    seen = set()
    for line, (bits, nl, nvalid, n) in zip(table[:NSPOT], spot_queries()):
        facts = "spot " + " ".join("%s=%d" % kv for kv in zip(names, bits)) + " nlayers=%d nvalid=%d n=%d" % (nl, nvalid, n)
        want = comp_image_before(*bits, nl, nvalid, n)
        assert line == facts + " -> " + want
        seen.add(want.split("(")[0] if not want.startswith("refused") else want)
    # every refusal and all sixteen instantiations occur
    assert {"refused: " + r for r in REFUSALS} <= seen and len(seen) == 4 + 16


def test_spot_refusal_order_of_the_plan(table):
    """the first failing condition wins: with every condition failing at once the first text comes out, and taking the
    failing conditions away from the front walks the texts in the order comp_image tested them (read off the program's table)"""
    rows = dict(line.split(" nlayers=3 nvalid=1264 n=7 -> ") for line in table[:NSPOT] if " nlayers=3 nvalid=1264 n=7 -> " in line)
    def row(from_buf, wfs_phase, wfs_all_int, cube, bincube, cog):
        return rows["spot from_buf=%d noise=0 cube=%d cog=%d no_atmos=0 no_dms=0 force_generic_spot=0 production_layout=1 "
                    "wfs_phase=%d bincube=%d wfs_all_int=%d" % (from_buf, cube, cog, wfs_phase, bincube, wfs_all_int)]
    assert row(1, 0, 0, 1, 0, 0) == "refused: " + REFUSALS[0]
    assert row(0, 0, 0, 1, 0, 0) == "refused: " + REFUSALS[1]
    assert row(0, 0, 1, 1, 0, 0) == "refused: " + REFUSALS[2]
    assert row(1, 1, 0, 1, 0, 0) == "refused: " + REFUSALS[2]
    assert row(0, 0, 1, 0, 0, 0) == "refused: " + REFUSALS[3]
    assert row(0, 0, 1, 0, 0, 1) == "k_wfs_spot_fast<3, false, false>(cog=1) grid=316x7 block=256"


def test_refusal_texts_are_the_header_s():
    """every refusal text in the header is, byte for byte, one comp_image passed to fail -- and nothing else is there"""
    with open(os.path.join(CSRC, "aomarl_stage_plan_host.h")) as fh:
        text = fh.read()
    body = text[text.index("spot_refusal_text"):text.index("enum SpotFamily")]
    got = [s for s in re.findall(r'return "([^"]*)";', body) if s]
    assert got == list(REFUSALS)


def test_target_plans_are_what_target_psf_decided(table):
    """every line of plan_target: rows kernel, grids, dynamic LDS bytes and finish kernel of the three branches it replaced"""
    names = ("from_buf", "production_layout", "force_valu_target", "force_generic_target")
    seen = set()
    for line, (bits, hw, npsf, pd, nl, nblk, n) in zip(table[NSPOT:NSPOT + NTARGET], target_queries()):
        facts = "target hw=%d npsf=%d pupdiam=%d nlayers=%d " % (hw, npsf, pd, nl) + " ".join("%s=%d" % kv for kv in zip(names, bits)) + \
                " nblk=%d n=%d" % (nblk, n)
        want = target_psf_before(hw, npsf, pd, nl, *bits, nblk, n)
        assert line == facts + " -> " + want
        seen.add(want.split(" ")[0])
    assert seen == {"k_target_rows_fast<1>", "k_target_rows_fast<3>", "k_target_rows_mfma<true>", "k_target_rows_mfma<false>",
                    "k_target_rows<true>", "k_target_rows<false>"}
