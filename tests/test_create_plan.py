"""What aomarl_create derives from a descriptor (csrc/aomarl_create_plan_host.h), CPU side: the stand-alone program around
the host-only plan under the address and undefined-behaviour sanitizers -- every table of its generated systems against
brute-force definitions, one descriptor per refusal --, the plan against the pinned table of what the function it
replaced produced, and refusals through the real ABI, which now precede the first HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ao_marl_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "create_plans.txt")
CASES = 59


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("create_plan") / "create_plan_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(CSRC, "create_plan_host_check.cpp")])
    out = subprocess.run([exe, "--table"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def test_host_check_builds_and_passes(table):
    """every accepted case keeps the invariants, every refused one gives its message"""
    assert table[-1] == "create_plan_host_check: ok (%d cases)" % CASES


def test_plan_is_the_pinned_table(table):
    """scalars, host values and every table's size, hash and places, line for line: the first section recorded from
    aomarl_create as it stood before the plan, the second (the inputs that crashed it) from the plan"""
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    assert os.path.getsize(GOLDEN) < 64 * 1024
    while want[0].startswith("#"):          # where the file comes from
        want.pop(0)
    got = table[:-1]
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, "line %d: %r, pinned %r" % (bad[0] + 1, got[bad[0]], want[bad[0]])
    assert len(got) == len(want)
    assert sum(line.startswith("case ") for line in want) == CASES
    marker = [i for i, line in enumerate(want) if line.startswith("# from here on")]
    assert len(marker) == 1 and all(line.startswith(("case ", "  refused: ")) for line in want[marker[0] + 1:])
    # the cases the issue names, read off the pinned table itself
    blocks = {}
    for line in want:
        if line.startswith("case "):
            name = line[5:]
            blocks[name] = []
        elif not line.startswith("#"):
            blocks[name].append(line)

    def flag(name, key):
        words = " ".join(l for l in blocks[name] if l.startswith("  sys ")).split()
        return int(words[words.index(key) + 1])

    assert [flag(n, "fused_ok") for n in ("one_layer_pd32_pad0", "three_layers_pd64_pad8_disc_shared_ab_big_screen",
                                          "three_layers_pd48_odd_tiles")] == [1, 1, 1]
    assert [flag(n, "fused_ok") for n in ("two_layers", "halfwin_4", "grey_pupil", "window_offset_off_by_one")] == [0, 0, 0, 0]
    assert flag("three_layers_pd48_odd_tiles", "ntiles") == 3
    assert flag("fractional_offset_skips_window_tests", "wfs_all_int") == 0
    assert flag("one_layer_pd32_pad0", "otf_ok") == 1 and flag("dm_pitch_12", "otf_ok") == 0
    shared = [l for l in blocks["three_layers_pd64_pad8_disc_shared_ab_big_screen"] if l.startswith("  table layers[")]
    assert any(l.endswith("-> layers[0].AB layers[1].AB") for l in shared) and any(l.endswith("-> layers[2].AB") for l in shared)
    assert any("layers[0].ABt" in l for l in shared) and not any("layers[2].ABt" in l for l in shared)


@pytest.fixture(scope="module")
def smallest():
    """(library, SimArrays) of the smallest geometry of geometry_cases"""
    from ao_marl_amd import libaomarl
    from tests import geometry_cases
    if not os.path.exists(libaomarl.LIB_PATH):
        libaomarl.build()
    name = min(geometry_cases.CASES, key=lambda k: geometry_cases.CASES[k].nxsub)
    return libaomarl.load(), geometry_cases.build(name)[2]


def _phasemap_not_a_tile(d, s, keep):
    pm = np.array(s.phasemap, dtype=np.int32).reshape(-1).copy()       # [pdiam^2][nvalid]
    pm[17 * s.nvalid + 2] += 1
    keep.append(pm)
    d.phasemap = pm.ctypes.data_as(C.POINTER(C.c_int32))


def _wfs_window_leaves_screen(d, s, keep):
    d.layers[0].wfs_xoff = float(s.screen_dim[0])


def _null_halfxy(d, s, keep):
    d.halfxy = None


@pytest.mark.parametrize("breakit, message", [
    (_phasemap_not_a_tile, "phasemap of sub-aperture 2 is not a contiguous tile"),
    (_wfs_window_leaves_screen, "WFS window leaves screen 0"),
    (_null_halfxy, "null host array in descriptor"),
], ids=["phasemap_not_a_tile", "wfs_window_leaves_screen", "null_halfxy"])
def test_refusals_through_the_abi_need_no_gpu(smallest, breakit, message):
    """one field of a good descriptor broken at a time: rc 1, the pinned message, no context -- on a machine without a
    GPU, because the plan refuses before anything is allocated"""
    from ao_marl_amd import libaomarl
    lib, s = smallest
    d, keep = libaomarl.make_desc(s)
    breakit(d, s, keep)
    ctx = C.c_void_p()
    assert lib.aomarl_create(C.byref(d), C.byref(ctx)) == 1
    assert lib.aomarl_last_error().decode() == message
    assert not ctx.value
    with open(GOLDEN) as fh:
        assert ("  refused: " + message) in fh.read().splitlines()
