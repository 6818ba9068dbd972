"""tests/geometry_cases.py on the CPU: every case builds on the branch it is there for, the float64 ray-trace agrees with
the oracle's fp32 one within its derived bound (before any GPU result is compared with it), and the Python mirror of
the library's eligibility rules sends each case where tests/test_gpu_geometries.py expects it."""
import numpy as np
import pytest

from oracle import aoref
from tests import geometry_cases as gc
from tests import helpers

NAMES = list(gc.CASES)


@pytest.fixture(scope="module")
def built():
    return {name: gc.build(name) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_case_builds_with_its_facts(built, name):
    ps, sysm, s = built[name]          # gc.build asserted the table's facts
    case = gc.CASES[name]
    assert ps.p_tel.diam == pytest.approx(0.2 * case.nxsub) and ps.p_atmos.nscreens == len(case.alt)
    assert s.nactu == sum(d.ntotact for d in s.dms) and s.nslope == 2 * s.nvalid
    assert all(len(ix) == len(iy) for ix, iy in zip(s.istx, s.isty))


def _fields(s, rng):
    """Random screens with structure at every scale down to the pixel (an interpolation error shows), random shapes."""
    screens = []
    for d in s.screen_dim:
        y, x = np.mgrid[0:d, 0:d] / float(d)
        scr = 3.0 * np.sin(5.0 * x + 3.0 * y) + rng.normal(0, 1.0, size=(d, d))
        screens.append(scr.astype(np.float32))
    return screens


@pytest.mark.parametrize("name", NAMES)
def test_oracle_raytrace_matches_float64(built, name):
    _, _, s = built[name]
    rng = np.random.default_rng(21)
    o = helpers.CalSim(s)
    screens = _fields(s, rng)
    for l, scr in enumerate(screens):
        o.screens[l][:] = scr
    o.comp_shapes(rng.normal(0, 100.0, size=s.nactu).astype(np.float32))       # mirrors of about a micron
    bound = gc.raytrace_bound(screens, o.dm_shapes)
    assert bound > 0
    for target in (False, True):
        for atm, dms in ((True, True), (True, False), (False, True)):
            (o.raytrace_target if target else o.raytrace_wfs)(atm=atm, dms=dms, reset=True)
            got = (o.tar_phase if target else o.wfs_phase).astype(np.float64)
            ref = gc.raytrace64(s, screens, o.dm_shapes, target, atm=atm, dms=dms)
            assert np.abs(ref).max() > 0.5
            d = float(np.abs(got - ref).max())
            print("%s %s atm=%d dms=%d: oracle - float64 = %.3g (bound %.3g)" % (name, "tar" if target else "wfs", atm, dms, d, bound))
            assert d <= bound, (name, target, atm, dms, d, bound)
    # the reference is not the oracle restated: a half-pixel shift of one offset moves it far past the bound
    if not gc.eligibility(s)["wfs_all_int"]:
        l = max(range(s.nscreens), key=lambda i: abs(s.wfs_atm_off[i][0] - round(s.wfs_atm_off[i][0])))
        keep = s.wfs_atm_off[l]
        s.wfs_atm_off[l] = (keep[0] + 0.5, keep[1])
        moved = gc.raytrace64(s, screens, o.dm_shapes, False)
        s.wfs_atm_off[l] = keep
        assert np.abs(moved - gc.raytrace64(s, screens, o.dm_shapes, False)).max() > 1e3 * bound


def _scalar_trace(field, nx, ny, xoff, yoff):
    """The conventions of the ray-trace written out pixel by pixel in Python floats."""
    N = field.shape[0]
    out = np.zeros((ny, nx))
    for y in range(ny):
        fy = float(np.float32(y) + np.float32(yoff))
        iy = int(np.floor(fy))
        for x in range(nx):
            fx = float(np.float32(x) + np.float32(xoff))
            ix = int(np.floor(fx))
            if ix < 0 or iy < 0 or ix >= N or iy >= N:
                continue
            wx, wy = fx - ix, fy - iy
            ix1, iy1 = min(ix + 1, N - 1), min(iy + 1, N - 1)
            out[y, x] = ((1 - wy) * ((1 - wx) * float(field[iy, ix]) + wx * float(field[iy, ix1])) +
                         wy * ((1 - wx) * float(field[iy1, ix]) + wx * float(field[iy1, ix1])))
    return out


@pytest.mark.parametrize("off", [(-1.25, 0.5), (4.75, -2.0), (5.5, 5.999), (0.0, 6.0), (7.3, -0.01)])
def test_float64_raytrace_edges(off):
    """Zero outside the field (the base pixel decides), the +1 neighbour clamped at the last row and column: the
    vectorised reference, the pixel-by-pixel definition and the oracle agree on windows that leave the field."""
    rng = np.random.default_rng(5)
    N, n = 12, 8
    field = rng.normal(0, 2.0, size=(N, N)).astype(np.float32)
    ref = np.zeros((n, n))
    gc._trace64(ref, field, off)
    want = _scalar_trace(field, n, n, off[0], off[1])
    assert np.abs(ref - want).max() < 1e-13
    assert (want == 0).any() and (want != 0).any()          # part of the window is outside, part inside
    got = np.zeros((n, n), dtype=np.float32)
    aoref.lib().aoref_raytrace(got.reshape(-1), n, n, field.reshape(-1), N, off[0], off[1], 0)
    assert np.abs(got - ref).max() <= 8.0 * 2.0 ** -24 * np.abs(field).max()
    assert np.array_equal(got == 0, ref == 0)


def test_eligibility_rules_send_each_case_to_its_branch(built):
    el = {name: gc.eligibility(built[name][2]) for name in NAMES}
    assert [n for n in NAMES if el[n]["fused_ok"]] == ["odd7", "odd17"]
    assert [n for n in NAMES if el[n]["tfast"]] == ["odd7", "odd17"]
    assert sum(el[n]["nt"] % 2 for n in NAMES) == 6 and sorted(el[n]["nt"] for n in NAMES) == [7, 9, 9, 13, 13, 17]
    # (all six tile counts are odd; the pair table's odd arm is read by the frame kernel of the two fused cases)
    assert [n for n in NAMES if el[n]["fused_ok"] and el[n]["nt"] % 2] == ["odd7", "odd17"]
    straddle = [n for n in NAMES if any(el[n]["layer_small"]) and not all(el[n]["layer_small"])]
    assert straddle == ["off13", "off13_dmalt"] and not el["off13"]["small_ok"]
    assert [n for n in NAMES if el[n]["small_ok"]] == ["odd7", "off9", "tar9"]
    # the mixed case: spots straight from the screens, PSF from the phase buffer
    assert [n for n in NAMES if el[n]["wfs_all_int"] and not el[n]["tar_all_int"]] == ["tar9"]
    assert [n for n in NAMES if not el[n]["wfs_all_int"]] == ["off9", "off13", "off13_dmalt"]
    # k_move_small's transposed [A|B] leading dimensions: 128 and 256 (production: 192 only)
    assert el["odd7"]["ldt"] == [128] and el["tar9"]["ldt"] == [192, 256] and el["off13"]["ldt"][:2] == [256, 256]
    # the 64-column loop of the target-row kernels: pd % 64 in {16, 48}, pd % 32 != 0
    assert sorted({built[n][2].pupdiam % 64 for n in NAMES}) == [16, 48]
    assert all(built[n][2].pupdiam % 32 != 0 for n in NAMES)
    assert {built[n][2].npsf for n in NAMES} == {256, 512, 1024}
    # more than one [A|B] class in one move
    assert all(len(set(built[n][2].screen_dim)) > 1 for n in ("off9", "tar9", "off13"))
