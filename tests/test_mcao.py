"""Multi-conjugate AO on the CPU (ao_marl_amd/mcao.py): the mirror's geometry, the sampling model against a scalar
restatement, the delay line against the simulator's, the ls reconstructor, the closed loop on the model path and the host
half under the sanitizers.  The device side is tests/test_gpu_mcao.py."""
import os
import subprocess

import numpy as np
import pytest

from ao_marl_amd import field as F
from ao_marl_amd import geometry as G
from ao_marl_amd import lgs as L
from ao_marl_amd import mcao as M
from ao_marl_amd import tomography as T
from tests import mcao_cases as mcs

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ao_marl_amd", "csrc")


# ------------------------------------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize("pupdiam", [mcs.SMALL, None])
def test_mirror_geometry(pupdiam):
    _, sysm, s = mcs.system_of(mcs.LAYERS_3, pupdiam)
    own = sysm.dms[0]
    for alts in (mcs.ALT_ONE, mcs.ALT_TWO):
        mirrors = mcs.mirrors_of(sysm, alts)
        for mir, h in zip(mirrors, alts):
            # an integer pitch (the system's own), the count from the pitch, the lattice centred on an even plane
            assert isinstance(mir.pitch, int) and mir.pitch == own.pitch and mir.alt == h
            patch = s.pupdiam + 2 * mcs.FIELD * G.ARCSEC2RAD * h / float(sysm.atm.pupixsize)
            assert mir.nact == int(np.ceil(patch / mir.pitch)) + 1 and mir.dim % 2 == 0
            c = (mir.dim - 1) / 2.
            assert np.allclose(np.sort(mir.xpos - c), -np.sort(-(mir.xpos - c))[::-1]) and abs((mir.xpos - c).sum()) < 1e-9
            assert abs((mir.ypos - c).sum()) < 1e-9
            steps = np.unique(np.diff(np.unique(mir.xpos)))
            assert steps.size == 1 and steps[0] == mir.pitch
            # every actuator within rad_out kept, none dropped inside; cobs = 0: the centre is there
            r = np.hypot(mir.xpos - c, mir.ypos - c)
            rad_out = ((mir.nact - 1) / 2. + 1.44) * mir.pitch
            assert r.max() <= rad_out and r.min() < mir.pitch
            nx = mir.nact + 4
            g = (np.arange(nx) - (nx - 1) / 2.) * mir.pitch
            assert mir.ntotact == int(np.sum(np.hypot(*np.meshgrid(g, g)) <= rad_out))
            # the lattice and the grid agree with the actuators' corners; every patch lies inside the plane
            assert np.array_equal(mir.grid[(mir.j1 - mir.j1min) // mir.pitch, (mir.i1 - mir.i1min) // mir.pitch],
                                  np.arange(mir.ntotact))
            assert np.count_nonzero(mir.grid >= 0) == mir.ntotact
            assert mir.i1min >= 0 and mir.i1.max() + mir.ss <= mir.dim and mir.j1min >= 0 and mir.j1.max() + mir.ss <= mir.dim
            assert mir.prof.shape == (mir.ss,) and abs(mir.prof.max()**2 - own.unitpervolt) < 1e-12
            assert (M.SHAPE_TILE + mir.ss - 2) // mir.pitch + 2 <= M.SHAPE_CELLS and mir.ss <= M.SHAPE_MAX_SS
        # every footprint of both constellations and of the line lies inside every plane
        mcs.assert_footprints_inside(sysm, mirrors, mcs.STARS_A, "wfs")
        off, dm1 = mcs.assert_footprints_inside(sysm, mirrors, mcs.STARS_B, "wfs")
        assert np.all(dm1[0] == 0) and np.allclose(dm1[1], -np.array(alts) / 90e3) and np.allclose(dm1[2], -np.array(alts) / 60e3)
        off, dm1 = mcs.assert_footprints_inside(sysm, mirrors, mcs.LINE, "pupil")
        assert np.all(dm1 == 0) and off.dtype == np.float32 and dm1.dtype == np.float32
        for m, mir in enumerate(mirrors):
            assert np.all(off[0, m] == (mir.dim - s.pupdiam) / 2.)
            shift = 20. * G.ARCSEC2RAD * mir.alt / float(sysm.atm.pupixsize)
            assert abs(off[4, m, 0] - off[0, m, 0] - shift) < 1e-4 and off[4, m, 1] == off[0, m, 1]
    with pytest.raises(ValueError, match="star 0 at \\(60, 0\\) arcsec leaves mirror 0"):
        M.mirror_offsets(sysm, mcs.mirrors_of(sysm, mcs.ALT_ONE), [(60., 0., 90e3)], "wfs")
    with pytest.raises(ValueError, match="gsalt = 5000 m is not above mirror 0"):
        M.mirror_offsets(sysm, mcs.mirrors_of(sysm, mcs.ALT_ONE), [(0., 0., 5000.)], "wfs")
    with pytest.raises(ValueError, match="alt = -1"):
        M.altitude_mirror(sysm, -1., 10.)
    with pytest.raises(ValueError, match="pitch = 7.5"):
        M.altitude_mirror(sysm, 1000., 10., pitch=7.5)


def test_mirror_at_altitude_zero_sits_on_the_systems_lattice():
    """alt = 0 with the ground pitch: the system's own stack-array actuators are actuators of the mirror, at the same
    places about the centre and with the same profile under them (the system leaves out what the obstruction hides)"""
    _, sysm, s = mcs.system_of(mcs.LAYERS_3, mcs.SMALL)
    own = sysm.dms[0]
    mir = M.altitude_mirror(sysm, 0., mcs.FIELD, coupling=float(sysm.params.p_dms[0].coupling))
    assert mir.pitch == own.pitch and mir.nact == sysm.params.p_dms[0].nact and mir.ss == own.influsize
    mine = {(float(x), float(y)) for x, y in zip(mir.xpos - (mir.dim - 1) / 2., mir.ypos - (mir.dim - 1) / 2.)}
    theirs = {(float(x), float(y)) for x, y in zip(own.xpos - sysm.geom.cent, own.ypos - sysm.geom.cent)}
    assert theirs <= mine and len(theirs) == own.ntotact and 0 <= len(mine) - len(theirs) <= 9
    assert all(np.hypot(*p) < 2 * mir.pitch for p in mine - theirs)
    infl = np.asarray(own.influ, dtype=np.float64)[:, :, 0]
    assert np.abs(np.outer(mir.prof, mir.prof) - infl).max() <= 4 * np.finfo(np.float32).eps * infl.max()


# ------------------------------------------------------------------------------------------------ 2. the models
def test_shape_model_against_the_definition():
    _, sysm, _ = mcs.system_of(mcs.LAYERS_3, mcs.SMALL)
    mir = mcs.mirrors_of(sysm, mcs.ALT_TWO)[0]
    com = mcs.commands([mir], 2, 1).astype(np.float64)
    got = M.mirror_shape_model(mir, com)
    assert got.shape == (2, mir.dim, mir.dim)
    for e in range(2):
        want = np.zeros((mir.dim, mir.dim))
        for a in range(mir.ntotact):
            want[mir.j1[a]:mir.j1[a] + mir.ss, mir.i1[a]:mir.i1[a] + mir.ss] += com[e, a] * np.outer(mir.prof, mir.prof)
        assert np.abs(got[e] - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(M.mirror_shape_model(mir, com, np.float32) - got).max() <= 1e-5 * np.abs(got).max()
    assert np.count_nonzero(M.mirror_shape_model(mir, np.zeros(mir.ntotact))) == 0
    with pytest.raises(ValueError, match="commands for"):
        M.mirror_shape_model(mir, com[:, :-1])


def _four_taps(shape, fx, fy):
    """the sampling rule written out for one coordinate"""
    dim = shape.shape[0]
    ix, iy = int(np.floor(fx)), int(np.floor(fy))
    if ix < 0 or iy < 0 or ix >= dim or iy >= dim:
        return 0.0
    wx, wy = fx - ix, fy - iy
    ix1, iy1 = min(ix + 1, dim - 1), min(iy + 1, dim - 1)
    top = (1 - wx) * shape[iy, ix] + wx * shape[iy, ix1]
    bot = (1 - wx) * shape[iy1, ix] + wx * shape[iy1, ix1]
    return (1 - wy) * top + wy * bot


def test_sampling_model():
    _, sysm, s = mcs.system_of(mcs.LAYERS_3, mcs.SMALL)
    mirrors = mcs.mirrors_of(sysm, mcs.ALT_TWO)
    rng = np.random.default_rng(3)
    shapes = [rng.standard_normal((m.dim, m.dim)) for m in mirrors]
    nn = s.n
    off, dm1 = M.mirror_offsets(sysm, mirrors, mcs.STARS_B, "wfs")
    base = rng.standard_normal((3, nn, nn))
    got = M.mirrors_add_model(base.copy(), shapes, off, dm1)
    c = (nn - 1) / 2.
    for k in range(3):
        for (y, x) in [(0, 0), (0, nn - 1), (nn - 1, 0), (nn - 1, nn - 1), (17, 33), (41, 42), (60, 5)]:
            want = base[k, y, x]
            for m, sh in enumerate(shapes):
                o, d = off[k, m].astype(np.float64), float(dm1[k, m])
                want = want + _four_taps(sh, (x + o[0]) + d * (x - c), (y + o[1]) + d * (y - c))
            assert got[k, y, x] == want, (k, y, x)
    # a natural star whose shift is a whole number of pixels: a shifted crop of the mirror's plane, exact
    mir = mirrors[0]
    per = G.ARCSEC2RAD * mir.alt / float(sysm.atm.pupixsize)
    off1, dm11 = M.mirror_offsets(sysm, [mir], [(12. / per, -9. / per, np.inf)], "wfs")
    x0, y0 = (mir.dim - nn) // 2 + 12, (mir.dim - nn) // 2 - 9
    assert float(off1[0, 0, 0]) == x0 and float(off1[0, 0, 1]) == y0 and dm11[0, 0] == 0
    crop = M.sample_model(shapes[0], off1[0, 0], dm11[0, 0], nn)
    assert np.array_equal(crop, shapes[0][y0:y0 + nn, x0:x0 + nn])
    assert np.array_equal(M.sample_model(shapes[0].astype(np.float32), off1[0, 0], dm11[0, 0], nn, np.float32),
                          shapes[0].astype(np.float32)[y0:y0 + nn, x0:x0 + nn])
    # the last line is clamped, outside gives 0
    small = rng.standard_normal((6, 6))
    edge = M.sample_model(small, (1.5, 5.25), 0., 5)                 # x: 1.5 .. 5.5, y: 5.25 .. 9.25
    assert edge[0, 0] == 0.5 * small[5, 1] + 0.5 * small[5, 2]       # row 5.25: rows 5 and the clamped 5
    assert edge[0, 4] == small[5, 5]                                 # column 5.5: columns 5 and the clamped 5
    assert np.all(edge[1:] == 0)                                     # rows 6.25 and beyond
    assert np.all(M.sample_model(small, (-1.5, 0.), 0., 5)[:, 0] == 0) and M.sample_model(small, (-1.5, 0.), 0., 5)[0, 2] != 0
    # the cone: the corner pixels move towards the centre by dm1 (nn - 1) / 2
    ramp = np.tile(np.arange(40.), (40, 1))
    cone = M.sample_model(ramp, (10., 10.), -0.1, 11)
    assert np.allclose(cone[5], 10. + np.arange(11) - 0.1 * (np.arange(11) - 5.))


def test_delay_line_is_the_simulators():
    """the model against the oracle's own command -> voltage over 6 frames of one random series, at the system's delay and
    at 0 and 2 frames: bit for bit in float32.  At a fractional delay the model's weights are the library's (float32
    arithmetic: 1.4f - 1) and the oracle's are float64 ones rounded (float32(1.4 - 1)), one unit in the last place apart:
    there the voltages agree to a rounding of the largest command."""
    from oracle import aoref
    _, _, s0 = mcs.system_of(mcs.LAYERS_3, mcs.SMALL)
    import copy
    rng = np.random.default_rng(6)
    series = (20. * rng.standard_normal((6, s0.nactu))).astype(np.float32)
    for delay in (float(s0.delay), 0.0, 2.0, 0.3, 1.4):
        s = copy.copy(s0)
        s.delay = delay
        o = aoref.OracleSim(s, seed=1)
        state = (np.zeros(s.nactu, dtype=np.float32), np.zeros(s.nactu, dtype=np.float32))
        for t in range(6):
            o.set_com(series[t])
            o.apply_control()
            v = M.delay_line_model(series[t:t + 1], delay, state)[0]
            assert v.dtype == np.float32
            if float(delay).is_integer():
                assert np.array_equal(v, o.voltage), (delay, t)
            else:
                assert np.abs(v - o.voltage).max() <= 2 * np.finfo(np.float32).eps * np.abs(series).max(), (delay, t)
        if float(delay).is_integer():
            assert np.array_equal(M.delay_line_model(series, delay)[5], o.voltage)
    assert [float(w) for w in M.delay_weights_f32(1.0)] == [0., 1., 0.]
    assert np.allclose(M.delay_weights_f32(1.4), (0., 0.6, 0.4)) and np.allclose(M.delay_weights_f32(0.3), (0.7, 0.3, 0.))


# ------------------------------------------------------------------------------------------------ 3. the reconstructor
def test_ls_reconstructor():
    rng = np.random.default_rng(1)
    U, _ = np.linalg.qr(rng.standard_normal((40, 12)))
    V, _ = np.linalg.qr(rng.standard_normal((12, 12)))
    sv = np.array([10., 8., 5., 3., 2., 1., 0.5, 0.2, 0.05, 0.02, 1e-3, 1e-6])
    D = (U * sv[None]) @ V.T
    for maxcond in (None, 1e9, 100., 15., 1.):
        W, ncut, s, Vt = M.ls_reconstructor(D, maxcond, return_svd=True)
        assert np.allclose(s, sv, rtol=1e-9, atol=1e-12)
        assert ncut == (0 if maxcond is None else int(np.sum(sv < sv[0] / maxcond)))
        kept = Vt[:12 - ncut]
        assert np.abs(W @ D @ kept.T - kept.T).max() <= 1e-8                  # the identity on the kept space
        if ncut:
            assert np.abs(W @ D @ Vt[12 - ncut:].T).max() <= 1e-8             # nothing of the cut space
    # the ridge filters: s / (s^2 + ridge mean(s^2))
    W, ncut = M.ls_reconstructor(D, 100., ridge=0.1)
    lam = 0.1 * np.mean(sv[:8]**2)
    assert ncut == 4 and np.allclose(np.linalg.svd(W, compute_uv=False)[:8], np.sort(sv[:8] / (sv[:8]**2 + lam))[::-1])
    # equilibrated: the same reconstruction of what the columns can reach, whatever their units
    scale = 10.**rng.uniform(-3, 3, 12)
    We, ncut_e = M.ls_reconstructor(D * scale[None], None, equilibrate=True)
    x = rng.standard_normal(12)
    assert ncut_e == 0 and np.allclose(We @ (D @ x), x / scale, rtol=1e-5, atol=1e-9)
    with pytest.raises(ValueError, match="maxcond"):
        M.ls_reconstructor(D, 0.5)
    with pytest.raises(ValueError, match="ridge"):
        M.ls_reconstructor(D, 10., ridge=-1.)


def test_ground_and_altitude_tilt_are_degenerate_for_natural_stars():
    """two natural stars, slopes by finite differences of the phase on a pupil: a tilt on the mirror at altitude gives every
    star the slopes ground tip-tilt gives -- the pair (ground tilt, -altitude tilt) is the smallest singular vector and
    falls into the cut space"""
    nn, dim, h_shift = 24, 64, (6, -5)
    yy, xx = np.mgrid[:dim, :dim].astype(np.float64)
    alt_modes = [xx - xx.mean(), yy - yy.mean(), (xx - xx.mean())**2 - (yy - yy.mean())**2, (xx - xx.mean()) * (yy - yy.mean())]
    alt_modes = [a / 30. for a in alt_modes]
    y, x = np.mgrid[:nn, :nn].astype(np.float64)
    g_modes = [(x - x.mean()) / 30., (y - y.mean()) / 30.]

    def slopes(ph):
        return np.concatenate([np.diff(ph, axis=1)[:, ::3].ravel(), np.diff(ph, axis=0)[::3].ravel()])
    cols = []
    for gm in g_modes:
        cols.append(np.concatenate([slopes(gm), slopes(gm)]))
    for am in alt_modes:
        per_star = []
        for sgn in (1, -1):                                          # the stars at +- the shift
            off = ((dim - nn) / 2. + sgn * h_shift[0], (dim - nn) / 2. + sgn * h_shift[1])
            per_star.append(slopes(M.sample_model(am, off, 0., nn)))
        cols.append(np.concatenate(per_star))
    D = np.stack(cols, axis=1)
    W, ncut, s, Vt = M.ls_reconstructor(D, 1e6, return_svd=True)
    assert ncut == 2 and s[-1] <= 1e-12 * s[0] and s[-2] <= 1e-12 * s[0] and s[-3] > 1e-3 * s[0]
    null = Vt[-2:]
    for v in null:
        assert np.abs(v[4:]).max() <= 1e-9                            # only tilts ...
        assert np.allclose(v[:2], -v[2:4], atol=1e-9)                 # ... ground against altitude, one to one
    assert np.abs(W @ D @ null.T).max() <= 1e-8


# ------------------------------------------------------------------------------------------------ 4. the loop on the CPU
@pytest.fixture(scope="module")
def cpu_sup():
    from ao_marl_amd.env import VecRlSupervisor
    from tests.oracle_vecsim import OracleVecSim
    return VecRlSupervisor(mcs.params(mcs.LAYERS_1, mcs.SMALL), dict(n_reverse_filtered_from_cmat=5), 2, device="cpu",
                           sim_factory=OracleVecSim)


def _own_path_sees_the_mirrors(sup, mc):
    """One more frame of the attached loop with the altitude mirrors in use: the oracle's own Strehl of that frame
    (frame(): raytrace_target + the mirrors; next_part_two: comp_strehl; get_strehl()) against direction (0, 0) of
    ScienceField(mirrors=mc) observed on the same state, between next_part_one and next_part_two.  The oracle's plane
    carries the float32 sampling of the mirrors, the field's the float64 one: about 4 roundings of values below 8 um,
    d = 4 x 6e-8 x 8 = 2e-6 um.  A Strehl exp(-sigma^2) moves by 2 sigma (2 pi d / lambda) relative, the variance by
    2 d / sqrt(variance); on top the 1e-6 of test_field.py's comparison with the oracle (its fp32 transform).  Without the
    mirrors the same state reads another Strehl."""
    assert np.abs(mc.alt_voltage).max() > 0
    on = mc.field([(0., 0.)])
    bare = F.ScienceField(sup.sim, [(0., 0.)], sysm=sup.sysm)          # (on the simulator: it does not know the attachment)
    sup.next_part_one()
    on.observe()
    bare.observe()
    sup.next_part_two(None, linear_control=True)
    own, own_fit = np.asarray(sup.get_strehl(do_fit=False), dtype=np.float64), np.asarray(sup.get_strehl(), dtype=np.float64)
    rec, d_um = on.record[:, 0], 2e-6
    for e in range(rec.shape[0]):
        sig = np.sqrt(rec[e, 2]) * 2 * np.pi / on.Lambda
        tol_s = 2 * sig * (2 * np.pi * d_um / on.Lambda) + 1e-6
        tol_v = 2 * d_um / np.sqrt(rec[e, 2]) + 1e-6
        pairs = ((rec[e, 0], own[e, 0], tol_s), (rec[e, 6], own_fit[e, 0], tol_s), (rec[e, 2], own[e, 2], tol_v))
        print("environment %d: field (SE, fitted, variance) %r  loop %r  relative bounds %.2e %.2e" % (
            e, [float(p[0]) for p in pairs], [float(p[1]) for p in pairs], tol_s, tol_v))
        for got, want, tol in pairs:
            assert abs(got - want) <= tol * abs(want)
        assert abs(bare.record[e, 0, 0] - own[e, 0]) > 0.01


def test_closed_loop_on_the_cpu_path(cpu_sup):
    """One layer at 8000 m, one mirror at 8000 m, constellation A, noise-free impulse kernels, 2 environments of the small
    system, 40 frames (the device test runs 300 at full size; 80 here would double a test that already takes a minute and
    a half, most of it the 842 pokes of the calibration): the ordering the device test asserts, on the model path."""
    sup = cpu_sup
    nframes = 40
    imp = L.impulse_kernels(sup.s.nvalid, sup.s.nfft)
    ngs, _ = F.strehl_against_angle(sup, mcs.LINE, nframes)
    lt = T.LaserTomography(sup, mcs.STARS_A, reconstructor="tomo", polc=True, noise=-1, kernels=imp)
    lt.calibrate()
    lt.start()
    ltao, _ = F.strehl_against_angle(sup, mcs.LINE, nframes)
    lt.stop()
    mc = M.MultiConjugate(sup, mcs.STARS_A, mirrors=[(8000.,)], field_radius=mcs.FIELD, noise=-1, kernels=imp)
    with pytest.raises(RuntimeError, match="calibrate\\(\\) first"):
        mc.start()
    with pytest.raises(NotImplementedError, match="polc"):
        M.MultiConjugate(sup, mcs.STARS_A, polc=True)
    with pytest.raises(NotImplementedError, match="set_atmosphere"):
        mc.set_atmosphere(r0=0.1)
    with pytest.raises(NotImplementedError, match="chosen at construction"):
        mc.set_reconstructor("mean")
    cg, ca = mc.calibrate()
    assert cg.shape == (sup.s.nactu, 4 * sup.s.nslope) and ca.shape == (mc.nact_total, 4 * sup.s.nslope)
    assert mc.ncut == int(np.sum(mc.svals < mc.svals[0] / mc.maxcond)) and mc.star_match <= 1e-3
    plain = F.ScienceField(sup, mcs.LINE)
    mc.start()
    try:
        with pytest.raises(RuntimeError, match="a MultiConjugate is attached"):
            plain.observe()
        mcao, _ = F.strehl_against_angle(sup, mcs.LINE, nframes, mirrors=mc)
        assert np.abs(mc.alt_com).max() > 0 and np.abs(mc.alt_voltage).max() > 0
        assert sup.get_slopes() is mc.est
        _own_path_sees_the_mirrors(sup, mc)
        sup.reset()
        assert np.abs(mc.alt_com).max() == 0 and all(np.abs(a).max() == 0 for a in mc.alt_shapes())
    finally:
        mc.stop()
    assert sup.lgs is None and sup.sensing is None
    print("field angle [arcsec]        " + "".join("%8.1f" % d[0] for d in mcs.LINE))
    for name, row in (("NGS integrator", ngs), ("LTAO tomo, polc", ltao), ("MCAO ls (%d of %d cut)" % (mc.ncut, mc.svals.size), mcao)):
        print("%-28s" % name + "".join("%8.4f" % v for v in row))
    assert mcao[3] > ngs[3] and mcao[3] > ltao[3]
    assert mcao[4] > ngs[4] and mcao[4] > ltao[4]
    assert mcao[4] / mcao[0] > ngs[4] / ngs[0]


# ------------------------------------------------------------------------------------------------ 5. the host program
def test_host_check_builds_and_passes(tmp_path):
    """mcao_host_check.cpp under the address and undefined-behaviour sanitizers: the validators' refusals, the shape
    launch's plan, the offset tables; the Makefile's host_check target runs it too"""
    exe = str(tmp_path / "mcao_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "mcao_host_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "mcao_host_check: ok"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    line = [ln for ln in mk.splitlines() if "_host_check.cpp" in ln][0]
    assert " mcao" in line and "aomarl_mcao.hip" in mk and "aomarl_mcao_host.h" in mk and "aomarl_mcao_sample.h" in mk
