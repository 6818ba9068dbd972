"""Mirror mis-registration on the CPU: the float64 model (ao_marl_amd.registration.trace_model) against independent
statements of what it must give (tests/registration_reference.py), the conditioning of the parameter sets the GPU
tests run (tests/registration_cases.py), the host half under the sanitizers, and every refusal by name."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from ao_marl_amd import registration as R
from tests import registration_cases as rc
from tests import registration_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ao_marl_amd", "csrc")


@pytest.fixture(scope="module")
def planes():
    """two planes with structure at every scale, sides no multiple of anything: [37, 37] and [41, 41]"""
    rng = np.random.default_rng(7)
    return [rng.standard_normal((37, 37)), rng.standard_normal((41, 41))]


IDENT = np.tile(R.IDENTITY_ROW, (2, 1))


# ------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("offsets", [((3.0, 5.0), (0.0, 2.0)), ((3.25, -1.5), (20.75, 19.5)), ((-4.0, 30.0), (1.5, 1.5))])
def test_identity_is_the_plain_rule(planes, offsets):
    """whole-pixel and fractional offsets, windows that leave the plane on either side and reach the clamped last line:
    the identity table gives the existing trace, in float64 and in float32 bit for bit"""
    nn = 24
    start = np.random.default_rng(1).standard_normal((nn, nn))
    for dt in (np.float64, np.float32):
        got = R.trace_model(nn, planes, offsets, IDENT, dtype=dt, start=start.astype(dt))
        want = ref.plain_trace(nn, planes, offsets, dtype=dt, start=start.astype(dt))
        assert got.dtype == dt and np.array_equal(got, want)
    assert np.abs(R.trace_model(nn, planes, offsets, IDENT)).max() > 0.5


@pytest.mark.parametrize("shift", [(0, 0), (4, -3), (-9, 2), (20, 25), (-40, 0), (13, 14)])
def test_integer_shifts_are_exact(planes, shift):
    nn, off = 24, (3.0, 5.0)
    row = R.rows_of(np.eye(2), np.array(shift, dtype=np.float64))
    got = R.trace_model(nn, planes[:1], [off], [row])
    want = ref.shifted_picture(planes[0], nn, off, shift)
    assert np.array_equal(got, want)
    if shift == (-40, 0):
        assert not got.any()                    # the plane has ended everywhere
    if shift == (-9, 2):
        assert not got[:, :6].any() and got[:, 6:].all()       # zeros exactly where it ends
    if shift == (13, 14):                       # x + 3 + 13 and y + 5 + 14 reach 36 = dim - 1 at x = 20, y = 17: the last
        assert got[:18, 20].all() and got[17, :21].all() and not got[:, 21:].any() and not got[18:].any()    # line, then nothing


def test_quarter_turn_is_exact(planes):
    nn, o = 24, 6
    q = np.array([[0.0, -1.0], [1.0, 0.0]])
    got = R.trace_model(nn, planes[:1], [(float(o), float(o))], [R.rows_of(q, np.zeros(2))])
    assert np.array_equal(got, ref.quarter_turn_picture(planes[0], nn, o))
    # four quarter turns are the identity
    pic = planes[0][o:o + nn, o:o + nn]
    for _ in range(4):
        pic = R.trace_model(nn, [pic], [(0.0, 0.0)], [R.rows_of(q, np.zeros(2))])
    assert np.array_equal(pic, planes[0][o:o + nn, o:o + nn])


def test_composition(planes):
    """two maps composed equal the map of the product: positions for any pair (float64 round-off), pictures for exact
    pairs wherever the outer map stays on the inner picture"""
    nn, off = 24, (6.0, 6.0)
    A1, t1 = R.registration_affine(0.013, -0.004, 0.3, 1.1, 0.0125)
    A2, t2 = R.registration_affine(-0.02, 0.007, -0.12, 0.93, 0.0125)
    outer, inner = R.rows_of(A1, t1), R.rows_of(A2, t2)
    both = R.compose_rows(outer, inner)
    uo, vo = R.sample_positions(nn, (0.0, 0.0), outer)          # where the outer trace looks on the inner picture
    c = 0.5 * (nn - 1)
    i = inner.astype(np.float64)
    u_nested = (c + off[0]) + i[0] * (uo - c) + i[1] * (vo - c) + i[4]
    v_nested = (c + off[1]) + i[2] * (uo - c) + i[3] * (vo - c) + i[5]
    u, v = (c + off[0]) + both[0] * (np.arange(nn)[None, :] - c) + both[1] * (np.arange(nn)[:, None] - c) + both[4], \
        (c + off[1]) + both[2] * (np.arange(nn)[None, :] - c) + both[3] * (np.arange(nn)[:, None] - c) + both[5]
    assert np.abs(u - u_nested).max() < 1e-12 and np.abs(v - v_nested).max() < 1e-12
    q = np.array([[0.0, -1.0], [1.0, 0.0]])
    outer, inner = R.rows_of(q, np.array([2.0, -3.0])), R.rows_of(q @ q, np.array([-1.0, 4.0]))
    first = R.trace_model(nn, planes[:1], [off], [inner])
    nested = R.trace_model(nn, [first], [(0.0, 0.0)], [outer])
    direct = R.trace_model(nn, planes[:1], [off], [R.compose_rows(outer, inner).astype(np.float32)])
    uo, vo = R.sample_positions(nn, (0.0, 0.0), outer)
    on = (uo >= 0) & (vo >= 0) & (uo < nn) & (vo < nn)
    assert on.sum() > nn * nn // 2 and (~on).any()
    assert np.array_equal(nested[on], direct[on]) and np.abs(direct[on]).max() > 0.5


def test_tip_tilt_rotated_is_the_rotated_pair():
    """a tip-tilt mirror turned by theta is the same mirror commanded with the pair turned by theta from x towards y"""
    dim, nn = 61, 24
    off = (0.5 * (dim - 1) - 0.5 * (nn - 1),) * 2               # the pupil's centre on the planes' zero
    g = (np.arange(dim) - 0.5 * (dim - 1)) * 0.03
    influ = np.stack([np.broadcast_to(g[None, :], (dim, dim)), np.broadcast_to(g[:, None], (dim, dim))], axis=-1)
    c0, c1, th = 0.7, -0.4, 0.21
    A, t = R.registration_affine(0.0, 0.0, th, 1.0, 0.0125)
    turned = R.trace_model(nn, [R.tt_plane(c0, c1, influ, np.float64)], [off], [R.rows_of(A, t)])
    r0, r1 = c0 * np.cos(th) - c1 * np.sin(th), c0 * np.sin(th) + c1 * np.cos(th)
    same = R.trace_model(nn, [R.tt_plane(r0, r1, influ, np.float64)], [off], [R.IDENTITY_ROW])
    # fp32 rounding of the table (cos, sin to 6e-8) times the largest lever (12 pixels of 0.03): 4e-8 at most
    assert np.abs(turned - same).max() < 1e-7 and np.abs(same).max() > 0.2
    rows64 = np.array([np.cos(th), np.sin(th), -np.sin(th), np.cos(th), 0, 0])
    u, v = (0.5 * (nn - 1) + off[0]) + rows64[0] * (np.arange(nn)[None, :] - 11.5) + rows64[1] * (np.arange(nn)[:, None] - 11.5), \
        (0.5 * (nn - 1) + off[1]) + rows64[2] * (np.arange(nn)[None, :] - 11.5) + rows64[3] * (np.arange(nn)[:, None] - 11.5)
    exact = R.bilinear(R.tt_plane(c0, c1, influ, np.float64), u, v)       # the same with the table in float64
    assert np.abs(exact - same).max() < 1e-14


def test_affine_helper_by_hand():
    # theta = 90 degrees, G = 2, (dx, dy) = (3, -1) pixels of 0.0125 m: A = [[0, 1/2], [-1/2, 0]], t = -A (3, -1)
    A, t = R.registration_affine(3 * 0.0125, -0.0125, np.pi / 2, 2.0, 0.0125)
    assert A.dtype == np.float32 and t.dtype == np.float32
    assert np.allclose(A, [[0, 0.5], [-0.5, 0]], atol=1e-7) and np.allclose(t, [0.5, 1.5], atol=1e-6)
    # 30 degrees, G = 0.8, (dx, dy) = (2, 1) pixels
    A, t = R.registration_affine(2 * 0.0125, 0.0125, np.pi / 6, 0.8, 0.0125)
    c, s = np.sqrt(3) / 2 / 0.8, 0.5 / 0.8
    assert np.array_equal(A, np.array([[c, s], [-s, c]]).astype(np.float32))
    assert np.array_equal(t, np.array([-(2 * c + s), 2 * s - c]).astype(np.float32))
    A, t = R.registration_affine(0.0, 0.0, 0.0, 1.0, 0.0125)
    assert np.array_equal(R.rows_of(A, t), R.IDENTITY_ROW)
    A, t = R.registration_affine(np.zeros(5), 0.0, np.linspace(0, 1, 5), 1.0, 0.0125)
    assert A.shape == (5, 2, 2) and t.shape == (5, 2)


# ------------------------------------------------------------------------------------------------ 2. the GPU cases
def test_cases_describe_the_10x10_system():
    from ao_marl_amd import geometry as G, params as P, system
    sysm = G.build_system(P.builtin(rc.NAME))
    s = system.from_system(sysm)
    assert (s.n, s.pupdiam) == (rc.GRIDS["wfs"][0], rc.GRIDS["tar"][0])
    assert tuple(int(d.dim) for d in s.dms) == rc.DIMS and [d.type for d in s.dms] == ["pzt", "tt"]
    assert tuple(map(tuple, s.wfs_dm_off)) == rc.GRIDS["wfs"][1] and tuple(map(tuple, s.tar_dm_off)) == rc.GRIDS["tar"][1]
    assert float(sysm.geom.pixsize) == rc.PIXSIZE and float(s.dms[0].pitch) == rc.PITCH
    b, sh = R.trace_bytes(s, target=False)
    assert b == 4 * 164 * 164 * (s.nscreens + 2) + 8 and sh == 8 * 164 * 164


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_case_conditioning(name):
    rows = rc.CASES[name]()
    assert rows.shape == (2, rc.NENV, 6) and rows.dtype == np.float32
    for k, dim in enumerate(rc.DIMS):
        R.check_rows(rows[k], dim)              # every case is one the library accepts
    c = rc.conditioning(rows)
    print(name, c)
    assert c["gap"] >= rc.MARGIN
    assert c["exact"] == (name != "fractional")
    assert c["leaves"] and c["last_row"] and c["last_col"] and c["negative"]
    # the environments of a case differ from one another
    for k in range(2):
        assert len({rows[k, e].tobytes() for e in range(rc.NENV)}) == rc.NENV


# ------------------------------------------------------------------------------------------------ 3. host half
def test_host_check_builds_and_passes(tmp_path):
    """dmreg_host_check.cpp under the address and undefined-behaviour sanitizers: every refusal of the validators by
    name, the four-parameter form, the coordinate bound; the Makefile's host_check target runs it too"""
    exe = str(tmp_path / "dmreg_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "dmreg_host_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "dmreg_host_check: ok"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    line = [ln for ln in mk.splitlines() if "_host_check.cpp" in ln][0]
    assert " dmreg;" in line and "aomarl_dmreg_host.h" in mk
    src = open(os.path.join(CSRC, "dmreg_host_check.cpp")).read()
    for word in ("not finite", "exceeds", "det A", "|t|", "environments", "mirror", "pipelined frame", "prefetched reset",
                 "target", "flags", "int32"):
        assert '"%s"' % word in src, word


def test_python_constants_are_the_headers():
    txt = open(os.path.join(CSRC, "aomarl_dmreg_host.h")).read()
    for name, val in (("DMREG_ROW", R.ROW), ("DMREG_A_MAX", R.A_MAX), ("DMREG_DET_MIN", R.DET_MIN),
                      ("DMREG_DET_MAX", R.DET_MAX), ("DMREG_T_DIMS", R.T_DIMS)):
        line = [ln for ln in txt.splitlines() if ln.startswith("#define %s " % name)][0]
        assert float(line.split()[2]) == float(val), name
    from ao_marl_amd import libaomarl as la
    names = {n for n, _, _ in la.SYMBOLS}
    assert {"aomarl_dmreg_create", "aomarl_dmreg_destroy", "aomarl_dmreg_set", "aomarl_dmreg_get",
            "aomarl_dmreg_trace"} <= names


# ------------------------------------------------------------------------------------------------ 4. refusals
def _fake_sup(**kw):
    """what DmRegistration reads of a supervisor, without a simulator behind it"""
    sim = SimpleNamespace(nenv=3)
    s = SimpleNamespace(dms=[SimpleNamespace(dim=258, type="pzt"), SimpleNamespace(dim=272, type="tt")])
    sup = SimpleNamespace(sim=sim, s=s, sysm=SimpleNamespace(geom=SimpleNamespace(pixsize=0.0125)), registration=None,
                          reset_prefetch=None, pure_delay_0=False, geo=None, pyramid=None, autoencoder=None,
                          keep_tar_image=False, keep_le_image=False, materialize_control=lambda: None)
    for k, v in kw.items():
        if k == "twin":
            sim._twin = v
        else:
            setattr(sup, k, v)
    return sup


def test_set_refusals_by_name():
    reg = R.DmRegistration(_fake_sup())
    assert reg.native is None and np.array_equal(reg.params["rows"], np.tile(R.IDENTITY_ROW, (2, 3, 1)))
    with pytest.raises(ValueError, match="not finite"):
        reg.set(0, dx=np.nan)
    with pytest.raises(ValueError, match="not finite"):
        reg.set(1, theta=[0.0, np.inf, 0.0])
    with pytest.raises(ValueError, match="G must be positive"):
        reg.set(0, G=0.0)
    with pytest.raises(ValueError, match=r"\|det A\|"):
        reg.set(0, G=2.5)
    with pytest.raises(ValueError, match=r"\|det A\|"):
        reg.set(0, G=[1.0, 0.3, 1.0])
    with pytest.raises(ValueError, match=r"\|t\|"):
        reg.set(0, dx=4.5 * 258 * 0.0125)
    with pytest.raises(ValueError, match="one value per environment"):
        reg.set(0, dx=[0.0, 1.0])
    with pytest.raises(IndexError, match="mirror"):
        reg.set(2, dx=0.0)
    with pytest.raises(IndexError, match="mirror"):
        reg.set_affine(-1, np.eye(2), np.zeros(2))
    with pytest.raises(ValueError, match="exceeds"):
        reg.set_affine(0, [[5.0, 0.0], [0.0, 0.2]], [0.0, 0.0])
    with pytest.raises(ValueError, match=r"\|det A\|"):
        reg.set_affine(0, [[1.0, 1.0], [1.0, 1.0]], [0.0, 0.0])
    with pytest.raises(ValueError, match="not finite"):
        reg.set_affine(0, np.eye(2), [0.0, np.nan])
    with pytest.raises(ValueError, match="must be"):
        reg.set_affine(0, np.eye(3), np.zeros(2))
    with pytest.raises(ValueError, match="one per environment"):
        reg.set_affine(0, np.tile(np.eye(2), (2, 1, 1)), np.zeros((2, 2)))
    # nothing of the refused calls stuck
    assert np.array_equal(reg.params["rows"], np.tile(R.IDENTITY_ROW, (2, 3, 1))) and not reg.params["dx"].any()
    with pytest.raises(RuntimeError, match="trace_model"):
        reg.trace(target=False)


def test_set_keeps_the_last_values_and_randomize_is_deterministic():
    reg = R.DmRegistration(_fake_sup())
    reg.set(0, dx=0.1, theta=[0.0, 0.01, 0.02])
    reg.set(0, dy=-0.05)                        # dx and theta stay (dmCompass.py:164-171)
    p = reg.params
    assert np.array_equal(p["dx"][0], [0.1] * 3) and np.array_equal(p["dy"][0], [-0.05] * 3)
    assert np.array_equal(p["theta"][0], [0.0, 0.01, 0.02]) and np.array_equal(p["G"], np.ones((2, 3)))
    A, t = R.registration_affine(0.1, -0.05, np.array([0.0, 0.01, 0.02]), 1.0, 0.0125)
    assert np.array_equal(p["rows"][0], R.rows_of(A, t)) and np.array_equal(p["rows"][1], np.tile(R.IDENTITY_ROW, (3, 1)))
    reg.set_affine(1, [[0.0, -1.0], [1.0, 0.0]], [1.0, 2.0])
    assert np.isnan(reg.params["theta"][1]).all() and np.array_equal(reg.params["rows"][1, 2], [0, -1, 1, 0, 1, 2])
    a, b = R.DmRegistration(_fake_sup()), R.DmRegistration(_fake_sup())
    a.randomize(5, shift_sigma_m=0.05, theta_sigma=0.01, G_sigma=0.02)
    b.randomize(5, shift_sigma_m=0.05, theta_sigma=0.01, G_sigma=0.02)
    assert np.array_equal(a.params["rows"], b.params["rows"]) and a.params["dx"].std() > 0.01
    assert len({a.params["rows"][0, e].tobytes() for e in range(3)}) == 3
    b.randomize(6, shift_sigma_m=0.05, theta_sigma=0.01, G_sigma=0.02)
    assert not np.array_equal(a.params["rows"], b.params["rows"])


@pytest.mark.parametrize("kw, exc, word", [
    (dict(twin=object()), RuntimeError, "frame pipeline"),
    (dict(reset_prefetch="same"), RuntimeError, "prefetched reset"),
    (dict(pure_delay_0=True), NotImplementedError, "modification_online"),
    (dict(geo=object()), RuntimeError, "GEO twin"),
    (dict(pyramid=object()), RuntimeError, "pyramid"),
    (dict(autoencoder=object()), RuntimeError, "denoiser"),
    (dict(keep_tar_image=True), RuntimeError, "keep_tar_image"),
    (dict(keep_le_image=True), RuntimeError, "keep_le_image"),
    (dict(registration=object()), RuntimeError, "attached already"),
])
def test_start_refusals_by_name(kw, exc, word):
    sup = _fake_sup(**kw)
    before = sup.registration
    with pytest.raises(exc, match=word):
        R.DmRegistration(sup).start()
    assert sup.registration is before


def test_start_and_stop_attach_and_detach():
    sup = _fake_sup()
    reg = R.DmRegistration(sup)
    assert reg.start() is reg and sup.registration is reg
    reg.stop()
    assert sup.registration is None
    reg.stop()                                  # a second stop is nothing


def test_other_features_refuse_an_attached_registration():
    from ao_marl_amd.pyramid import PyramidSensor
    from ao_marl_amd.roket import _roket_supervisor
    pyr = PyramidSensor.__new__(PyramidSensor)
    pyr.cmat = np.zeros((1, 1))
    pyr.sup = SimpleNamespace(pyramid=None, registration=object())
    with pytest.raises(RuntimeError, match="mis-registration"):
        pyr.start()
    sim = SimpleNamespace()
    sup = SimpleNamespace(sim=sim, prefetch_atmos=False, reset_prefetch=None, gain=0.4, modal_gains=None, geo=object(),
                          registration=object(), pure_delay_0=False, autoencoder=None)
    env = SimpleNamespace(supervisor=sup, rl_step=None, frame_pipeline=False)
    with pytest.raises(RuntimeError, match="mis-registration"):
        _roket_supervisor(env)
