"""The slopes-only fp32 frame kernel (moments from four matrix products, csrc/aomarl_spot_dev.h: spot_qf_moments)
against the float64 centre of gravity of the phase it receives (tests/phase_range.py: slopes64), on screens that pin
what the folded constants of its table decide: (i) a pure x tilt, (ii) a pure y tilt of another size and the other
sign -- axis and sign of both slopes -- and (iii) random tilts of up to +-6 revolutions per sub-aperture with a little
noise.  Every valid sub-aperture, edge and partly lit ones included, at the project's 1e-4 arcsec.

Shapes: the 10 x 10 system with 3 environments (not a multiple of 4: one wave of each workgroup repeats an
environment; the three cases in ONE frame) and the 40 x 40 system with 1 environment (three frames)."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import geometry as G, params, system  # noqa: E402
from tests import phase_range as pr  # noqa: E402

TOL = 1e-4                                                        # arcsec
NAME_RE = re.compile(r"k_frame_wave<\d+, \d+, true, false, false, false>")


def _screens(s, rng):
    """Layer 0 of the three cases [3, d, d] (um); the other layers stay flat."""
    d = s.screen_dim[0]
    lam, pd = float(s.wfs_lambda), int(s.pdiam)
    y, x = np.mgrid[0:d, 0:d].astype(np.float64)
    tilt_x = 1.3 * lam * x / pd                                   # +1.3 revolutions per sub-aperture along x
    tilt_y = -2.1 * lam * y / pd                                  # -2.1 along y
    nb = -(-d // pd)
    tx, ty = rng.uniform(-6.0, 6.0, size=(2, nb, nb))
    tx[0, 0], ty[0, 0], tx[-1, -1], ty[-1, -1] = 6.0, -6.0, -6.0, 6.0
    up = lambda a: np.kron(a, np.ones((pd, pd)))[:d, :d]          # noqa: E731
    rand = lam * (up(tx) * (x % pd) + up(ty) * (y % pd)) / pd + 0.05 * lam * rng.normal(size=(d, d))
    return np.stack([tilt_x, tilt_y, rand]).astype(np.float32)


def _run(name, nenv, groups):
    """groups: lists of case indices, one list per frame (len = nenv)."""
    from ao_marl_amd import libaomarl as la
    from ao_marl_amd.sim import HipSim
    s = system.from_system(G.build_system(params.builtin(name)), strehl_halfwin=8)
    s.cmat = np.zeros((s.nactu, s.nslope), dtype=np.float32)      # these frames never run the controller
    sim = HipSim(s, nenv=nenv, keep_phase=True)
    assert sim.frame_fused_available() and sim.dm_from_voltage_available()
    cases = _screens(s, np.random.default_rng(7))
    volts = torch.zeros((nenv, s.nactu), dtype=torch.float32, device="cuda")
    keep = la.get_precision()
    la.set_precision("f32")
    sim.set_option("force_f32_dft", 1)
    worst = {}
    try:
        for grp in groups:
            sim.set_screen(0, cases[grp])
            for l in range(1, s.nscreens):
                sim.set_screen(l, np.zeros((nenv, s.screen_dim[l], s.screen_dim[l]), np.float32))
            sim.comp_dm_shape(volts)
            sim.raytrace_wfs(atm=True, dms=True, reset=True)
            wfs = sim.t["wfs_phase"].cpu().numpy().copy()
            sim.set_com(volts)
            sim.apply_control(comp_voltage=False, defer_shape=True)
            sim.frame_fused(noise=False, write_bincube=False, cog=True)
            assert NAME_RE.fullmatch(sim.frame_kernel_name()), sim.frame_kernel_name()
            sl = sim.slopes.cpu().numpy().astype(np.float64)
            for e, case in enumerate(grp):
                ref = pr.slopes64(s, wfs[e])
                assert not np.isnan(ref).any()
                dx = float(np.abs(sl[e, :s.nvalid] - ref[:s.nvalid]).max())
                dy = float(np.abs(sl[e, s.nvalid:] - ref[s.nvalid:]).max())
                print("%s case %d: max |d slope| x %.3g, y %.3g arcsec (slopes up to %.3g)" % (name, case, dx, dy, np.abs(ref).max()))
                worst[case] = (dx, dy, ref, sl[e])
    finally:
        sim.set_option("force_f32_dft", -1)
        la.set_precision(keep)
    nv = s.nvalid
    for case, (dx, dy, ref, got) in worst.items():
        assert dx < TOL and dy < TOL, (name, case, dx, dy)
    # (i) and (ii) pin axis and sign only if the references are far from zero on the tilted axis, in every sub-aperture
    assert np.abs(worst[0][2][:nv]).min() > 100 * TOL and np.abs(worst[1][2][nv:]).min() > 100 * TOL
    assert (np.sign(worst[0][2][:nv]) == -np.sign(worst[1][2][nv:])).all()


def test_small_three_environments_one_frame():
    _run("production_sh_10x10_2m", 3, [[0, 1, 2]])


def test_large_one_environment_three_frames():
    _run("production_sh_40x40_8m_3layers", 1, [[0], [1], [2]])
