"""The science field on the CPU (ao_marl_amd/field.py): the offsets and their refusals, the trace against a scalar
restatement (tests/field_reference.py), FieldModel against numpy.fft.fft2, direction (0, 0) against the oracle's own Strehl
on the same state, the anisoplanatism of a frozen atmosphere, the refusals by name, and the host half under the
sanitizers.  The system is tests/tomo_cases.py's: 10x10, field declared at 25 arcsec, strehl_halfwin = 8."""
import copy
import os
import subprocess
import types

import numpy as np
import pytest

from ao_marl_amd import field as F
from ao_marl_amd import geometry as G
from tests import field_reference as ref
from tests import tomo_cases as tc

CSRC = os.path.join(os.path.dirname(os.path.abspath(F.__file__)), "csrc")
DIRS = [(0., 0.), (20., 0.), (-10., 15.), (7.3, -11.9)] + F.ring(16, 20.0)


# ------------------------------------------------------------------------------------------------ 1. offsets
@pytest.mark.parametrize("alts", [tc.LAYERS_3, tc.LAYERS_1])
def test_offsets_on_axis_are_the_targets(alts):
    ps, sysm, s = tc.system_of(alts)
    off = F.field_offsets(sysm, [(0., 0.)])
    want, _ = G.target_layer_offsets(ps.p_targets[0], sysm.atm, sysm.dms, sysm.geom, ps.p_tel)
    assert off.dtype == np.float32 and off.shape == (1, len(alts), 2)
    assert np.array_equal(off[0].astype(np.float64), np.asarray(want, dtype=np.float64))
    assert np.array_equal(off[0].astype(np.float64), np.asarray(s.tar_atm_off, dtype=np.float64))
    # a direction moves layer l by theta alt_l / pupixsize pixels, the ground layer not at all
    o2 = F.field_offsets(sysm, [(0., 0.), (20., -10.)])
    shift = np.array([20., -10.])[None, :] * G.ARCSEC2RAD * np.asarray(sysm.atm.alt)[:, None] / sysm.atm.pupixsize
    assert np.abs((o2[1] - o2[0]).astype(np.float64) - shift).max() <= 2e-5
    assert np.array_equal(o2[0], off[0])


def test_a_direction_beyond_the_declared_field_is_refused_with_the_radius():
    _, sysm, _ = tc.system_of(tc.LAYERS_3)
    with pytest.raises(ValueError, match=r"direction 1 at \(60, 0\) arcsec leaves screen 1 .* declare a field of radius 60 arcsec"):
        F.field_offsets(sysm, [(0., 0.), (60., 0.)])
    with pytest.raises(ValueError, match="radius 75 arcsec"):
        F.field_offsets(sysm, [(0., -74.2)])


@pytest.mark.parametrize("alts", [tc.LAYERS_3, tc.LAYERS_1])
def test_footprints_agree_with_the_refusal(alts):
    """every direction of the list passes and its footprint lies inside every screen; walking out along x, the first
    direction field_offsets refuses is the first whose footprint (the helper's) leaves a screen"""
    _, sysm, _ = tc.system_of(alts)
    dims = np.asarray(sysm.atm.dim_screens, dtype=np.float64)
    off = F.field_offsets(sysm, DIRS)
    fp = F.field_footprints(sysm, off)
    assert fp.shape == (len(DIRS), len(alts), 2, 2)
    assert fp.min() >= 0 and np.all(fp <= (dims - 1)[None, :, None, None])
    assert np.array_equal(fp[..., 1] - fp[..., 0], np.full(fp.shape[:3], sysm.geom.pupdiam - 1.0))
    base = np.asarray(sysm.targets[0].atm_off, dtype=np.float64)
    alt = np.asarray(sysm.atm.alt, dtype=np.float64)
    last_ok = None
    for r in np.arange(20.0, 120.0, 0.25):
        by_hand = (base + np.array([r, 0.]) * G.ARCSEC2RAD * alt[:, None] / sysm.atm.pupixsize).astype(np.float32)
        inside = bool(np.all(F.field_footprints(sysm, by_hand[None]) <= (dims - 1)[None, :, None, None]))
        try:
            F.field_offsets(sysm, [(r, 0.)])
            assert inside, r
            last_ok = r
        except ValueError:
            assert not inside, r
            break
    else:
        raise AssertionError("no direction up to 120 arcsec was refused")
    assert last_ok is not None and last_ok >= tc.FIELD          # the declared field is honoured
    print("layers %s: the largest direction along x the screens allow: %.2f arcsec" % (alts, last_ok))


# ------------------------------------------------------------------------------------------------ 2. the trace
def test_trace_model_against_the_scalar_restatement():
    """exactly equal in float64: fractional offsets, the on-axis whole-pixel ones, and a hand-made direction whose
    footprint crosses the last line (clamped) and leaves the screens (zero)"""
    _, sysm, s = tc.system_of(tc.LAYERS_3)
    rng = np.random.default_rng(7)
    screens = [rng.normal(size=(d, d)).astype(np.float32) for d in s.screen_dim]
    off = F.field_offsets(sysm, [(0., 0.), (7.3, -11.9), (-10., 15.)])
    pd = int(s.pupdiam)
    edge = np.array([[[d - pd + 1.5, d - pd - 3.25] for d in s.screen_dim]], dtype=np.float32)
    off = np.concatenate([off, edge])
    got = F.field_trace_model(screens, off, pd)
    want = ref.trace_planes(screens, off, pd)
    assert got.dtype == np.float64 and got.shape == (4, pd, pd)
    assert np.array_equal(got, want)
    assert np.all(got[3][:, -1] == 0) and np.abs(got[3][:, -2]).min() > 0          # beyond the last line / on it, clamped
    assert np.abs(got[1] - got[0]).max() > 1e-3 and np.abs(got[2] - got[0]).max() > 1e-3
    # whole-pixel offsets: the plain window of the screens
    o0 = off[0].astype(int)
    plain = sum(scr[oy:oy + pd, ox:ox + pd].astype(np.float64) for scr, (ox, oy) in zip(screens, o0))
    assert np.array_equal(got[0], plain)
    # float32: the device's arithmetic, close to the definition
    g32 = F.field_trace_model(screens, off, pd, dtype=np.float32)
    # (a position below 256 is rounded by at most 2^-17 pixel per axis; a pixel apart the screens differ by at most `step`)
    step = max(max(np.abs(np.diff(scr, axis=0)).max(), np.abs(np.diff(scr, axis=1)).max()) for scr in screens)
    assert g32.dtype == np.float32 and np.abs(g32 - got).max() <= len(screens) * 2.0**-16 * step + 1e-6


# ------------------------------------------------------------------------------------------------ 3. the PSF side
@pytest.fixture(scope="module")
def model():
    _, _, s = tc.system_of(tc.LAYERS_3)
    return F.FieldModel(s), s


def _fft_window(m, phase):
    a = np.zeros((m.npsf, m.npsf), dtype=np.complex128)
    a[:m.pd, :m.pd] = m.pupil * np.exp(2j * np.pi * np.asarray(phase, dtype=np.float64) / m.Lambda)
    p = np.abs(np.fft.fft2(a))**2
    idx = np.arange(-m.hw, m.hw) % m.npsf
    return p[np.ix_(idx, idx)]


def test_model_window_against_fft2(model):
    m, s = model
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:m.pd, :m.pd] / float(m.pd)
    phases = [0.15 * rng.normal(size=(m.pd, m.pd)) + 0.4 * xx - 0.2 * yy, 2.5 * rng.normal(size=(m.pd, m.pd))]
    for ph in phases:
        got, want = m.window(ph), _fft_window(m, ph)
        assert got.shape == (m.W, m.W) == (16, 16)
        assert np.abs(got - want).max() <= 1e-12 * want.max()
        assert abs(m.variance(ph) - np.var(ph[np.asarray(s.spupil) != 0])) <= 1e-12 * np.var(ph)
    # a flat phase (any piston): Strehl 1, the peak at zero frequency, the fit's gain 1
    rec, le = m.new_state()
    m.commit(np.full((m.pd, m.pd), 0.37), rec, le)
    assert abs(rec[0] - 1.0) <= 1e-12 and abs(rec[6] - 1.0) <= 1e-9 and rec[2] <= 1e-24 and rec[5] == 0 and rec[4] == 1
    assert np.argmax(le) == m.hw * m.W + m.hw
    # the long exposure of two frames is the mean of their windows
    rec, le = m.new_state()
    w0 = m.commit(phases[0], rec, le)
    se0 = rec[0]
    w1 = m.commit(phases[1], rec, le)
    assert rec[4] == 2 and np.abs(le / rec[4] - 0.5 * (w0 + w1)).max() <= 1e-12 * w0.max()
    assert abs(rec[1] - (0.5 * (w0 + w1)).max() / m.ref_peak) <= 1e-12 and abs(rec[0] - w1.max() / m.ref_peak) <= 1e-15
    assert abs(rec[3] - (m.variance(phases[0]) + m.variance(phases[1]))) <= 1e-12 * rec[3] and se0 == w0.max() / m.ref_peak
    assert rec[7] >= rec[1] and rec[6] >= rec[0]
    # the window's tilt: a peak off the centre, and a peak on the edge says so in slot 5
    rec, le = m.new_state()
    m.commit(-m.Lambda * m.hw * (xx * m.pd) / m.npsf, rec, le)                 # exp(2 pi i (-hw) x / npsf): column 0
    assert rec[5] == 1.0 and rec[6] == rec[0]
    # float32, the yardstick of the device: close to the definition
    m32 = F.FieldModel(s, dtype=np.float32)
    assert np.abs(m32.window(phases[0]) - m.window(phases[0])).max() <= 1e-4 * m.window(phases[0]).max()
    assert abs(m32.variance(phases[0]) - m.variance(phases[0])) <= 1e-4 * m.variance(phases[0])


def test_sinc_fit_cases():
    assert F.sinc_gain(0.5, 1.0, 0.5) == pytest.approx(1.0, abs=1e-12)        # symmetric: the maximum is the peak
    assert F.sinc_gain(1.0, 0.0, 1.0) == 1.0 and F.sinc_gain(1.0, 1.0, 1.0) == 1.0
    for w, x0 in ((1.2, 0.3), (2.0, -0.25), (0.6, 0.45)):                       # samples of a sinc: the fit finds its peak
        y = [np.sinc(w * (x - x0) / np.pi) for x in (-1., 0., 1.)]
        assert F.sinc_gain(*y) == pytest.approx(1.0 / y[1], rel=1e-9)
    img = np.zeros((8, 8))
    img[3, 4], img[3, 3], img[3, 5], img[2, 4], img[4, 4] = 1.0, 0.6, 0.8, 0.7, 0.7
    m, fit, edge = F.fit_peak(img)
    assert m == 1.0 and not edge and fit == pytest.approx(F.sinc_gain(0.6, 1.0, 0.8) * F.sinc_gain(0.7, 1.0, 0.7))
    img[0, 0] = 2.0
    assert F.fit_peak(img) == (2.0, 2.0, True)


# ------------------------------------------------------------------------------------------------ 4. on a CPU simulator
@pytest.fixture(scope="module")
def cpu_sup():
    """a VecRlSupervisor on the oracle (one OracleSim per environment), one layer at 8000 m, 2 environments"""
    from ao_marl_amd.env import VecRlSupervisor
    from tests.oracle_vecsim import OracleVecSim
    return VecRlSupervisor(tc.params(tc.LAYERS_1), dict(n_reverse_filtered_from_cmat=5), 2, device="cpu",
                           sim_factory=OracleVecSim)


def test_on_axis_agrees_with_the_oracle(cpu_sup):
    """direction (0, 0) on the state as it stands against the oracle's own raytrace_target + comp_strehl of that state:
    strehl_se, strehl_se_fit, the phase variance.  The oracle computes in fp32 (cosf / sinf of the unwrapped angle, an
    fp32 FFT): 1e-6 relative."""
    sup = cpu_sup
    sup.reset()
    for _ in range(3):
        sup.next_part_one()
        sup.next_part_two(None, linear_control=True)
    fld = F.ScienceField(sup, [(0., 0.), (12., 5.)])
    keep = [o.tar_phase.copy() for o in sup.sim.sims]
    fld.observe()
    assert all(np.array_equal(k, o.tar_phase) for k, o in zip(keep, sup.sim.sims))           # it only reads
    rec = fld.record
    worst = 0.0
    for e, o in enumerate(sup.sim.sims):
        o.raytrace_target()
        o.reset_strehl()
        o.comp_strehl()
        pairs = ((rec[e, 0, 0], o.strehl_se), (rec[e, 0, 6], o.strehl_se_fit), (rec[e, 0, 2], o.phase_var))
        for got, want in pairs:
            worst = max(worst, abs(got - want) / abs(want))
        print("environment %d: field %r  oracle %r" % (e, [float(p[0]) for p in pairs], [float(p[1]) for p in pairs]))
    print("largest relative difference to the oracle: %.3e" % worst)
    assert worst <= 1e-6
    st = fld.strehl()
    assert st.shape == (2, 2, 4) and np.all(st[:, 1, 0] < st[:, 0, 0])          # 13 arcsec off axis: a lower Strehl
    assert np.array_equal(fld.strehl(do_fit=False)[..., 0], rec[..., 0])
    assert fld.le_image().shape == (2, 2, 16, 16) and np.all(rec[..., 4] == 1)
    fld.reset(env_begin=1)
    assert np.all(fld.record[1] == 0) and np.all(fld.record[0] == rec[0]) and np.all(fld.le_image()[1] == 0)
    # run(): frames of the supervisor's loop with an observe behind each
    fld.reset()
    out = fld.run(2)
    assert out.shape == (2, 2, 4) and np.all(fld.record[..., 4] == 2)


def test_frozen_atmosphere_decorrelates_with_the_angle(cpu_sup):
    """one layer at 8000 m, the atmosphere as the reset left it, the mirrors flat: the variance over the pupil of the
    phase difference to the on-axis direction is zero at (0, 0), positive and increasing along line(20, 5), in every
    environment (the structure function of the layer at a shift of 0.19 m per 5 arcsec)"""
    sup = cpu_sup
    sup.reset()
    fld = F.ScienceField(sup, F.line(20, 5))
    planes = fld.trace(atm=True, dms=True)
    assert planes.shape == (2, 5, sup.s.pupdiam, sup.s.pupdiam)
    assert np.array_equal(planes, fld.trace(atm=True, dms=False))          # flat mirrors add nothing
    lit = np.asarray(sup.s.spupil) != 0
    for e in range(2):
        v = np.array([np.var((planes[e, d] - planes[e, 0])[lit]) for d in range(5)])
        print("environment %d: variance of the difference to the axis [um^2] %s" % (e, np.array2string(v, precision=5)))
        assert v[0] == 0.0 and np.all(np.diff(v) > 0)
    fld.observe()
    st = fld.strehl()
    assert np.all(st[:, 1:, 0] != st[:, :1, 0])                             # the directions see different phases


def test_closed_loop_strehl_falls_with_the_angle_on_the_model(cpu_sup):
    """the statement the device test relies on, on the CPU path with fewer frames: the integrator's long-exposure Strehl
    along line(20, 5) is non-increasing within the spread between the environments and strictly lower at 20 arcsec"""
    sup = cpu_sup
    sup.reset()
    fld = F.ScienceField(sup, F.line(20, 5))
    le = fld.run(30)[..., 1]
    mean, spread = le.mean(0), le.max(0) - le.min(0)
    print("long-exposure Strehl along the line %s, spread between the environments %s" % (
        np.array2string(mean, precision=4), np.array2string(spread, precision=4)))
    assert np.all(mean[1:] <= mean[:-1] + np.maximum(spread[1:], spread[:-1])) and mean[4] < mean[0]


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_by_name(cpu_sup):
    sup = cpu_sup
    with pytest.raises(ValueError, match="ndir = 0"):
        F.ScienceField(sup, [])
    with pytest.raises(ValueError, match=r"direction 1: \(nan, 3\) is not finite"):
        F.ScienceField(sup, [(0., 0.), (float("nan"), 3.)])
    with pytest.raises(ValueError, match="not finite"):
        F.field_offsets(sup.sysm, [(np.inf, 0.)])
    with pytest.raises(ValueError, match="pairs"):
        F.ScienceField(sup, [(1., 2., 3.)])
    for lam in (0., -1.65, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="Lambda = .* must be positive and finite"):
            F.ScienceField(sup, [(0., 0.)], Lambda=lam)
        with pytest.raises(ValueError, match="Lambda"):
            F.FieldModel(sup.s, Lambda=lam)
    with pytest.raises(ValueError, match="radius 70 arcsec"):
        F.ScienceField(sup, [(0., 0.), (0., 70.)])
    # a mirror at altitude, by name
    s2 = copy.copy(sup.s)
    s2.dms = [copy.copy(d) for d in sup.s.dms]
    s2.dms[0].alt = 4000.
    high = types.SimpleNamespace(s=s2, nenv=2, device="cpu", sims=sup.sim.sims)
    with pytest.raises(NotImplementedError, match="ScienceField: a mirror conjugated to 4000 m"):
        F.ScienceField(high, [(0., 0.)], sysm=sup.sysm)
    # a simulator needs its geometry; the CPU path needs one oracle per environment
    bare = types.SimpleNamespace(s=sup.s, nenv=2, device="cpu")
    with pytest.raises(ValueError, match="pass sysm"):
        F.ScienceField(bare, [(0., 0.)])
    fld = F.ScienceField(bare, [(0., 0.)], sysm=sup.sysm)
    with pytest.raises(NotImplementedError, match="one oracle per environment"):
        fld.observe()
    with pytest.raises(NotImplementedError, match="one oracle per environment"):
        fld.trace()
    with pytest.raises(RuntimeError, match="built on a simulator"):
        fld.run(1)
    ok = F.ScienceField(sup, [(0., 0.)], Lambda=2.2)
    assert ok.Lambda == 2.2 and ok.model.Lambda == 2.2
    with pytest.raises(ValueError, match=r"environments 1 \.\. \+2 of 2"):
        ok.observe(env_begin=1, env_count=2)
    # it is no attachment: nothing on the supervisor knows it
    from ao_marl_amd import attachments
    assert not any("field" in k for k in attachments.TABLE) and sup.sensing is None and sup.control_law is None


def test_helpers():
    assert F.line(20, 5) == [(0., 0.), (5., 0.), (10., 0.), (15., 0.), (20., 0.)]
    g = F.grid(10, 3)
    assert len(g) == 9 and g[0] == (-10., -10.) and g[4] == (0., 0.) and g[2] == (10., -10.) and g[8] == (10., 10.)
    r = F.ring(16, 20.0)
    assert len(r) == 16 and r[0] == (20., 0.) and np.allclose(np.hypot(*np.array(r).T), 20.0)
    assert F.grid(5, 1) == [(0., 0.)] and F.line(5, 1) == [(0., 0.)]


# ------------------------------------------------------------------------------------------------ 6. the host half
def test_host_check_builds_and_passes(tmp_path):
    """field_host_check.cpp under the address and undefined-behaviour sanitizers: the validators' refusals, the plan of
    the launches, the kernels' offset table; the Makefile's host_check target runs it too"""
    exe = str(tmp_path / "field_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "field_host_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "field_host_check: ok"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    line = [ln for ln in mk.splitlines() if "_host_check.cpp" in ln][0]
    assert " field " in line and "aomarl_field.hip" in mk and "aomarl_field_host.h" in mk
