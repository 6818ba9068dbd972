"""The pair walk of the slopes-only fp32 frame kernel (csrc/aomarl_frame.hip): two fully lit sub-aperture tiles of a
pair are computed as ONE interleaved instruction block (pair_block), every other pair tile by tile (tile()).  One frame
with non-zero voltages, every layer non-flat and random tilts of up to +-6 revolutions per sub-aperture, against float64
of the phase the kernel receives (the kept ray-traced phases): slopes (tests/phase_range.py: slopes64) at 1e-4 arcsec,
short-exposure Strehl ratio -- the PSF rows of every stripe -- at 2e-5 SR + 1e-7 and the phase variance -- the stripe
sums and the lit count it is divided by -- at 1e-4 relative, the bounds of tests/parity_stages.py and
tests/test_gpu_phase_range.py for the same quantities.

Shapes: the 10 x 10 system with 3 environments (not a multiple of 4: one wave of each workgroup repeats an environment)
and the 40 x 40 system with 1.  Their tile counts (10, 40) are even and their pupils symmetric, so no stripe of theirs
has an odd number of lit tiles: odd7 of tests/geometry_cases.py (7 tiles per stripe, the smallest of
tests/test_gpu_geometries.py with a fused frame) is the third, with 1 environment.

Coverage: the library has no call that hands its tile tables out, so tile_info and pair_info are rebuilt here by the
rule of csrc/aomarl_create_plan_host.h (create_plan_tiles) from the pupil and the sub-apertures' places, and the
systems together must contain every kind of pair the walk distinguishes."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import geometry as G, params, system  # noqa: E402
from tests import geometry_cases as gc  # noqa: E402
from tests import phase_range as pr  # noqa: E402

TOL = 1e-4                                                        # arcsec
NAME_RE = re.compile(r"k_frame_wave<\d+, \d+, true, false, false, false>")
LIT, FULL, SUB = 0x10000, 0x20000, 0x40000
KINDS = ("full + full", "full + partial", "lit + unlit", "tile without a sub-aperture", "odd stripe")
SYSTEMS = (("production_sh_10x10_2m", 3), ("production_sh_40x40_8m_3layers", 1), ("odd7", 1))


def _system(name):
    ps = gc.param_set(name) if name in gc.CASES else params.builtin(name)
    s = system.from_system(G.build_system(ps), strehl_halfwin=8)
    s.cmat = np.zeros((s.nactu, s.nslope), dtype=np.float32)      # this frame never runs the controller
    return s


def tile_tables(s):
    """(tile_info [nt, nt], pairs: per stripe the list of (info_a, info_b)) by the rule of create_plan_tiles."""
    pd, pad = int(s.pupdiam), (int(s.n) - int(s.pupdiam)) // 2
    nt = pd // 16
    m = np.asarray(s.spupil).reshape(pd, pd) != 0
    blocks = m.reshape(nt, 16, nt, 16)
    lit, full = blocks.any(axis=(1, 3)), blocks.all(axis=(1, 3))
    tsub = np.full((nt, nt), -1, dtype=np.int64)
    p0 = np.asarray(s.phasemap).reshape(s.pdiam * s.pdiam, s.nvalid)[0]
    for i in range(s.nvalid):
        x0, y0 = int(p0[i]) % int(s.n) - pad, int(p0[i]) // int(s.n) - pad
        assert x0 % 16 == 0 and y0 % 16 == 0 and tsub[y0 // 16, x0 // 16] < 0
        tsub[y0 // 16, x0 // 16] = i
    info = np.where(lit, LIT, 0) | np.where(full, FULL, 0) | np.where(tsub >= 0, SUB | LIT | np.maximum(tsub, 0), 0)
    pairs = []
    for r in range(nt):
        row = []
        for g in range((nt + 1) // 2):
            va = int(info[r, 2 * g])
            vb = int(info[r, 2 * g + 1]) if 2 * g + 1 < nt else 0
            if (va | vb) & LIT:
                row.append((va if va & LIT else 0, vb if vb & LIT else 0))
        pairs.append(row)
    return info, pairs


def pair_kinds(s):
    info, pairs = tile_tables(s)
    k = set()
    block = LIT | FULL | SUB
    for r, row in enumerate(pairs):
        for va, vb in row:
            fa, fb = (va & block) == block, (vb & block) == block
            if fa and fb:
                k.add("full + full")
            if (fa and (vb & LIT) and not vb & FULL) or (fb and (va & LIT) and not va & FULL):
                k.add("full + partial")
            if bool(va & LIT) != bool(vb & LIT):
                k.add("lit + unlit")
            if any((v & LIT) and not v & SUB for v in (va, vb)):
                k.add("tile without a sub-aperture")
        if int(((info[r] & LIT) != 0).sum()) % 2:
            k.add("odd stripe")
    return k


def _screens(s, rng, nenv):
    """[layer][nenv, d, d] (um): layer 0 random tilts of up to +-6 sensor revolutions per sub-aperture with a little
    noise (one draw per environment), the other layers smooth ripples of a few tenths of a wave."""
    lam, pd = float(s.wfs_lambda), int(s.pdiam)
    out = []
    for l in range(s.nscreens):
        d = int(s.screen_dim[l])
        y, x = np.mgrid[0:d, 0:d].astype(np.float64)
        scr = np.empty((nenv, d, d), np.float32)
        for e in range(nenv):
            if l == 0:
                nb = -(-d // pd)
                tx, ty = rng.uniform(-6.0, 6.0, size=(2, nb, nb))
                tx[0, 0], ty[0, 0], tx[-1, -1], ty[-1, -1] = 6.0, -6.0, -6.0, 6.0
                up = lambda a: np.kron(a, np.ones((pd, pd)))[:d, :d]          # noqa: E731
                f = lam * (up(tx) * (x % pd) + up(ty) * (y % pd)) / pd + 0.05 * lam * rng.normal(size=(d, d))
            else:
                kx, ky, ph = rng.uniform(0.02, 0.11), rng.uniform(0.02, 0.11), rng.uniform(0, 6.28)
                f = 0.3 * lam * np.sin(kx * x + ph) * np.cos(ky * y) + 0.02 * lam * rng.normal(size=(d, d))
            scr[e] = f
        out.append(scr)
    return out


def _run(name, nenv):
    from ao_marl_amd import libaomarl as la
    from ao_marl_amd.sim import HipSim
    s = _system(name)
    sim = HipSim(s, nenv=nenv, keep_phase=True)
    assert sim.frame_fused_available() and sim.dm_from_voltage_available()
    rng = np.random.default_rng(11)
    screens = _screens(s, rng, nenv)
    assert all(float(np.abs(sc).max()) > 0 for sc in screens)
    volts = torch.from_numpy(rng.normal(0, 0.3, size=(nenv, s.nactu)).astype(np.float32)).cuda()
    keep = la.get_precision()
    la.set_precision("f32")
    sim.set_option("force_f32_dft", 1)
    try:
        for l, sc in enumerate(screens):
            sim.set_screen(l, sc)
        sim.comp_dm_shape(volts)
        sim.raytrace_wfs(atm=True, dms=True, reset=True)
        sim.raytrace_target(atm=True, dms=True, reset=True)
        wfs, tar = sim.t["wfs_phase"].cpu().numpy().copy(), sim.t["tar_phase"].cpu().numpy().copy()
        sim.set_com(volts)
        sim.apply_control(comp_voltage=False, defer_shape=True)
        sim.reset_strehl()
        sim.frame_fused(noise=False, write_bincube=False, cog=True)
        assert NAME_RE.fullmatch(sim.frame_kernel_name()), sim.frame_kernel_name()
        sim.comp_strehl()
        sl = sim.slopes.cpu().numpy().astype(np.float64)
        st = sim.strehl.cpu().numpy().astype(np.float64)
    finally:
        sim.set_option("force_f32_dft", -1)
        la.set_precision(keep)
    fails = []
    for e in range(nenv):
        ref = pr.slopes64(s, wfs[e])
        assert not np.isnan(ref).any()
        sr64, var64 = pr.strehl64(s, tar[e]), pr.phase_var64(s, tar[e])
        d_sl = float(np.abs(sl[e] - ref).max())
        d_sr, d_var = abs(st[e, 0] - sr64), abs(st[e, 2] - var64) / var64
        print("%s env %d: max |d slope| %.3g arcsec (slopes up to %.3g); SE Strehl %.6g, float64 %.6g, |d| %.3g (bound %.3g); "
              "phase variance relative |d| %.3g" % (name, e, d_sl, np.abs(ref).max(), st[e, 0], sr64, d_sr, 2e-5 * sr64 + 1e-7, d_var))
        if not d_sl < TOL:
            fails.append((name, e, "slopes", d_sl))
        if not d_sr < 2e-5 * sr64 + 1e-7:
            fails.append((name, e, "SE Strehl", st[e, 0], sr64))
        if not d_var < 1e-4:
            fails.append((name, e, "phase variance", st[e, 2], var64))
    assert not fails, fails


def test_the_systems_contain_every_kind_of_pair():
    found = {}
    for name, _ in SYSTEMS:
        found[name] = pair_kinds(_system(name))
        print("%s: %s" % (name, sorted(found[name])))
    assert set().union(*found.values()) == set(KINDS), found
    assert "full + full" in found["production_sh_10x10_2m"] and "full + full" in found["production_sh_40x40_8m_3layers"]


@pytest.mark.parametrize("name,nenv", SYSTEMS)
def test_pair_walk_against_float64(name, nenv):
    _run(name, nenv)
