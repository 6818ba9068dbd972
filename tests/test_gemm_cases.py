"""The cases of the GEMM conformance tests (tests/gemm_cases.py) hold what the device tests rely on, checked without a
GPU: exactness is a property of the inputs, the float64 reference is itself exact, every instantiation is reached --
and the host side of k_gemm_p's configuration (aomarl_gemm_p_host.h) passes its stand-alone check program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gemm_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ao_marl_amd", "csrc")


def _all_nt():
    for wm, wn in gc.P_TILES:
        yield gc.nt_axes(wm, wn), gc.nt_cases(gc.KERNEL_P, wm, wn)
    yield gc.nt_axes(2, 2), gc.nt_cases(gc.KERNEL_NT)
    yield gc.nt_axes(2, 2), gc.nt_cases(gc.KERNEL_NT_H)


def test_case_tables_name_the_headers_instantiations():
    hp = open(os.path.join(CSRC, "aomarl_gemm_p_host.h")).read()
    menu = re.search(r"#define GP_FOR_EACH_TILE\(X\)(.*)", hp).group(1)
    assert tuple((int(a), int(b)) for a, b in re.findall(r"X\((\d), (\d)\)", menu)) == gc.P_TILES
    hg = open(os.path.join(CSRC, "aomarl_gemm_g.h")).read()
    tiles = re.findall(r"return k_gemm_g<(\d), (\d), AK, BK>;", hg)
    assert sorted((int(a), int(b)) for a, b in tiles) == sorted(gc.G_TILES)


def test_every_pair_of_axis_values_occurs():
    for axes, cases in _all_nt():
        assert len(cases) >= 150 and gc.uncovered_pairs(cases, axes) == []
    for wm, wn in gc.G_TILES:
        for ak, bk in gc.G_FORMS:
            assert gc.uncovered_pairs(gc.g_cases(wm, wn, ak, bk), gc.g_axes(wm, wn, ak, bk)) == []
    for G in gc.BATCHED_KGROUPS:
        assert gc.uncovered_pairs(gc.batched_cases(G), gc.batched_axes()) == []


def test_case_lists_are_reproducible():
    a = gc.pairwise(gc.nt_axes(3, 2), seed=5)
    b = gc.pairwise(gc.nt_axes(3, 2), seed=5)
    assert a == b and a != gc.pairwise(gc.nt_axes(3, 2), seed=6)


def test_every_instantiation_is_reached():
    counts = gc.instantiation_counts()
    # 8 k_gemm_p tiles (each also split), the two 64 x 64 kernels, 4 tiles x 4 forms of k_gemm_g with their mask and
    # column-sum epilogues, 4 transposes x 3 k-group counts of k_gemm_batched_gen
    assert len(counts) == 2 * 8 + 2 + 16 * 2 + 8 + 12
    assert [k for k, v in counts.items() if v == 0] == []


def _exact_in_float32(a, b):
    """the float32 product, bit for bit the float64 one"""
    p32 = a.astype(np.float32) @ b.astype(np.float32)
    p64 = a @ b
    return p32.dtype == np.float32 and np.array_equal(p32.astype(np.float64), p64)


def test_nt_cases_are_exact_by_construction():
    n = 0
    for _, cases in _all_nt():
        for c in cases:
            assert gc.exactness_margin(c["K"], c["alpha"], c["beta"]) < 2 ** 24
            d = gc.nt_data(c)
            assert _exact_in_float32(d["a"], d["b"].T), c
            a32 = np.float32(c["alpha"]) * (d["a"].astype(np.float32) @ d["b"].astype(np.float32).T)
            r32 = a32 + np.float32(c["beta"]) * d["c0"].astype(np.float32) if c["beta"] else a32
            assert r32.dtype == np.float32 and np.array_equal(r32.astype(np.float64), d["ref"]), c
            # the layout: NaN between K and the leading dimension, a sentinel round the M x N window
            assert np.isnan(d["A"][:, c["K"]:]).all() and np.isnan(d["B"][:, c["K"]:]).all()
            assert not np.isnan(d["A"][:, :c["K"]]).any() and d["lda"] % 4 == 0 and d["ldb"] % 4 == 0
            assert (d["Cbuf"][c["M"]:] == gc.SENTINEL).all() and (d["Cbuf"][:, c["N"]:] == gc.SENTINEL).all()
            assert np.isnan(d["Cbuf"][:c["M"], :c["N"]]).all() == (c["beta"] == 0.0)
            assert not np.isnan(d["want"]).any()
            # the slabs of a split add up to the product, whatever the chunk
            for kchunk in (32, 96):
                nz = -(-c["K"] // kchunk)
                assert np.array_equal(gc.slab_products(d["a"], d["b"], kchunk, nz).sum(0), d["a"] @ d["b"].T)
            n += 1
    assert n >= 10 * 150


def test_grouped_and_batched_cases_are_exact_by_construction():
    for wm, wn in gc.G_TILES:
        for ak, bk in gc.G_FORMS:
            for c in gc.g_cases(wm, wn, ak, bk):
                assert gc.exactness_margin(c["K"], 1.0, 1.0) < 2 ** 24
                d = gc.g_data(c)
                assert all(_exact_in_float32(d["a"][g], d["b"][g]) for g in range(c["groups"])), c
                assert d["lda"] % 4 == 0 and d["ldb"] % 4 == 0
                if not ak:
                    assert c["M"] % 4 == 0
                if not bk:
                    assert c["N"] % 4 == 0
                    assert np.array_equal(d["b"].astype(np.float32).sum(1).astype(np.float64), d["b"].sum(1))
                assert not np.isnan(d["want"]).any() and (d["want_cs"][:, c["N"]:] == gc.SENTINEL).all()
                if c["mask"]:
                    m = d["mask"][:, :, :c["N"]]
                    assert (m > 0).any() and (m == 0).any() and (m < 0).any() or c["M"] * c["N"] < 3
    for G in gc.BATCHED_KGROUPS:
        for c in gc.batched_cases(G):
            assert gc.exactness_margin(c["K"], 1.0, 2.0) < 2 ** 24
            d = gc.batched_data(c)
            assert all(_exact_in_float32(d["a"][g], d["b"][g]) for g in range(c["batch"])), c
            assert (d["lda"] % 4 == 0, d["ldb"] % 4 == 0) == (bool(c["aligned_a"]), bool(c["aligned_b"]))
            assert not np.isnan(d["want"]).any()


def test_probe_structs_match_the_header():
    """GemmProbe / GemmGArgs are the header's structs field by field: size and the offset of EVERY field, from a probe
    compiled with the host compiler."""
    import tempfile
    from ao_marl_amd import libaomarl as la
    structs = (("aomarl_gemm_probe", la.GemmProbe), ("aomarl_gemm_g_args", la.GemmGArgs))
    items = []
    for cname, cls in structs:
        items.append("sizeof(%s)" % cname)
        items += ["offsetof(%s,%s)" % (cname, f[0]) for f in cls._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aomarl.h"\nint main(){size_t v[]={%s};'
           'for(size_t i=0;i<sizeof(v)/sizeof(v[0]);i++)printf("%%zu ",v[i]);return 0;}\n' % ",".join(items))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "p"),
                               os.path.join(d, "p.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "p")]).decode().split()]
    want = []
    for _, cls in structs:
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f[0]).offset for f in cls._fields_]
    assert len(want) > 50 and out == want
    # and the header has no field the binding lacks
    hdr = open(os.path.join(ROOT, "include", "aomarl.h")).read()
    for cname, cls in structs:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"[*\s,]([A-Za-z_][A-Za-z0-9_]*)\s*(?=[,;])", body)
        assert names == [f[0] for f in cls._fields_], cname


def test_gemm_p_host_check_program(tmp_path):
    """aomarl_gemm_p_host.h and aomarl_gemm_plan_host.h through their stand-alone program: every configuration
    gemm_p_pick returns over the grid of shapes, K = 1 .. 4100, with and without a workspace, is one k_gemm_p can run,
    and every plan launch_gemm_nt makes over that grid x alignment x options is one its kernels and reduces can run
    (see the program's header).  The plans of the loop's own shapes are the pinned ones (tests/golden/gemm_plans.txt,
    recorded from the launcher before it had a plan)."""
    exe = str(tmp_path / "gemm_p_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe,
                           os.path.join(CSRC, "gemm_p_host_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 2
    assert lines[0].startswith("gemm_p_host_check: ok (3968800 configurations")
    assert lines[1].startswith("gemm_plan: ok (388876800 plans")
    r = subprocess.run([exe, "--plans"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    want = open(os.path.join(ROOT, "tests", "golden", "gemm_plans.txt")).read()
    assert len(want.splitlines()) == 960 and r.stdout.decode() == want
