"""Pyramid sensor on the CPU: the geometry against the fixture written from the reference's own init code
(tests/golden/pyr_geom.npz, tools/gen_golden_pyr.py), the invariants of the float64 model (ao_marl_amd/pyramid.py:
PyramidModel), the refusals, and the host half of the native object under the sanitizers.

Flat wavefront, per-point slopes: the quarter images of the model are added coherently, so a point's four pixels also
hold the tails of the other three images and of the transform's periodic copies.  A point's slope vanishes on a flat
wavefront only where every image sees a point-symmetric surrounding: an open field stop (the reference's stop is centred
half a pixel off the zero frequency) and the four images and their copies on ONE regular lattice, which is
Nfft = 4 pupdiam (tiny A; pupdiam 64 / nxsub 16).  There the bound is 1e-10 s_scale.  On the other geometries (tiny B,
Nfft = 16 / 3 pupdiam; the 10x10 system, Nfft = 3.2 pupdiam) single points read up to 0.024 and 0.060 s_scale on a flat
wavefront -- what the reference slopes are for -- and what symmetry leaves exact is the MEAN slope: bound 1e-10 s_scale,
with the open stop, on every geometry."""
import os
import subprocess

import numpy as np
import pytest

from ao_marl_amd import geometry as G
from ao_marl_amd import params as P
from ao_marl_amd.pyramid import PyramidModel, PyramidSensor, pyr_noise
from tests import pyramid_cases as pc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ao_marl_amd", "csrc")
OPEN = 100.0        # arcsec: a field stop wider than the whole focal plane


@pytest.fixture(scope="module")
def golden():
    with np.load(pc.GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize("tag", pc.TAGS)
def test_geometry_equals_the_fixture(golden, tag):
    z = golden
    geom, sz, pg, tel, w = pc.build(z, tag)
    s = lambda k: pc.scalar(z, tag, k)  # noqa: E731
    expect = {"tinyA": (128, 4), "tinyB": (256, 4), "s10_10": (512, 16), "s10_20": (512, 8)}[tag]
    assert (sz.Nfft, sz.nrebin) == expect == (s("Nfft"), s("nrebin"))
    assert (geom.n, geom.pupdiam, sz.pdiam, pg.nvalid) == (s("n"), s("pupdiam"), s("pdiam"), s("nvalid"))
    for k, v in (("qpixsize", sz.qpixsize), ("pixsize", sz.pixsize), ("nphotons", pg.nphotons), ("s_scale", pg.s_scale),
                 ("pyr_scale_pos", pg.pyr_scale_pos)):
        assert abs(v / s(k) - 1) <= 1e-6, k
    assert pg.s_offset == 0.
    assert np.array_equal(pg.validsubsx, z[tag + "_validsubsx"]) and np.array_equal(pg.validsubsy, z[tag + "_validsubsy"])
    assert pg.validsubsx.size == 4 * pg.nvalid
    for k in ("pyr_cx", "pyr_cy"):
        ref = z["%s_%s" % (tag, k)]
        assert np.abs(getattr(pg, k) - ref).max() <= 1e-6 * np.abs(ref).max()
    planes = dict(submask=pg.submask, halfxy=pg.halfxy.astype(np.float32), sincar=pg.sincar, isvalid=pg.isvalid,
                  mpupil=pg.mpupil)
    for k, v in planes.items():
        assert pc.sha(v) == str(z["%s_sha_%s" % (tag, k)]), k
        if "%s_%s" % (tag, k) in z:
            ref = z["%s_%s" % (tag, k)]
            assert v.shape == ref.shape
            if k in ("submask", "isvalid", "mpupil"):
                assert np.array_equal(v, ref), k
            else:
                assert np.abs(v - ref).max() <= 1e-6 * np.abs(ref).max(), k
    if tag.startswith("tiny"):
        assert "%s_submask" % tag in z and "%s_halfxy" % tag in z      # whole arrays for the tiny cases


def test_sizes_of_the_issue():
    tel2, tel8 = P.Param_tel(diam=2., cobs=0.12), P.Param_tel(diam=8., cobs=0.12)
    for nx, nrebin in ((10, 16), (20, 8), (40, 4)):
        sz = G.pyr_sizes(P.Param_wfs(type="pyrhr", nxsub=nx, Lambda=0.5), tel2, 160)
        assert (sz.Nfft, sz.nrebin) == (512, nrebin)
    assert G.pyr_sizes(P.Param_wfs(type="pyrhr", nxsub=40, Lambda=0.5), tel8, 640).Nfft == 2048


# ------------------------------------------------------------------------------------------------ 2. the model
@pytest.fixture(scope="module")
def open_models(golden):
    """tag -> (geom, pg, tel, model, flat image, flat slopes): 16 points of 3 lambda / D, open stop; computed once"""
    out = {}
    for tag in ("tinyA", "tinyB", "s10_10"):
        geom, sz, pg, tel, w = pc.build(golden, tag, fssize=OPEN)
        assert pg.pyr_cx.size == 16 and w.pyr_ampl == 3.
        m = PyramidModel(pg, method=1)
        img, sl = m.measure(np.zeros((1, pg.n, pg.n)))
        out[tag] = (geom, pg, tel, m, img[0], sl[0])
    return out


def _regular(golden):
    """pupdiam 64, nxsub 16, obstruction 0.12: Nfft = 256 = 4 pupdiam"""
    tel = P.Param_tel(diam=2., cobs=0.12)
    _, w, ittime = pc.params_of(golden, "tinyA", nxsub=16, fssize=OPEN)
    geom = G.pupil_geometry(64, tel)
    sz = G.pyr_sizes(w, tel, geom.pupdiam)
    assert sz.Nfft == 4 * geom.pupdiam
    return G.pyr_geometry(w, sz, geom, tel, ittime)


def test_flat_wavefront_slopes(golden, open_models):
    for tag, (geom, pg, tel, m, img, sl) in open_models.items():
        nv = pg.nvalid
        mean = max(abs(sl[:nv].mean()), abs(sl[nv:].mean()))
        print("%s: flat wavefront, largest |slope| %.3e s_scale, largest |mean slope| %.3e s_scale"
              % (tag, np.abs(sl).max() / pg.s_scale, mean / pg.s_scale))
        assert mean <= 1e-10 * pg.s_scale, tag
        if pg.Nfft == 4 * geom.pupdiam:
            assert np.abs(sl).max() <= 1e-10 * pg.s_scale, tag
    assert open_models["tinyA"][1].Nfft == 4 * open_models["tinyA"][0].pupdiam
    pg = _regular(golden)
    _, sl = PyramidModel(pg, method=1).measure(np.zeros((1, pg.n, pg.n)))
    assert np.abs(sl).max() <= 1e-10 * pg.s_scale


def test_flat_wavefront_flux(open_models):
    for tag, (geom, pg, tel, m, img, sl) in open_models.items():
        assert abs(img.sum() / pg.nphotons - 1) <= 1e-9, tag
        q = img[pg.validsubsx, pg.validsubsy].reshape(4, pg.nvalid).sum(axis=1)
        share = q.sum() / img.sum()
        print("%s: share of the flux on the valid pixels %.4f" % (tag, share))
        assert share >= 0.6, tag
        assert np.abs(q / q.sum() - 0.25).max() <= 1e-9, tag


def test_a_field_stop_loses_light(golden):
    geom, sz, pg, tel, w = pc.build(golden, "tinyA")
    img, _ = PyramidModel(pg).measure(np.zeros((1, pg.n, pg.n)))
    assert 0.5 * pg.nphotons < img.sum() < pg.nphotons * (1 - 1e-4)


@pytest.mark.parametrize("axis", [1, 0])
def test_tilt_response(open_models, axis):
    for tag, (geom, pg, tel, m, img, sl) in open_models.items():
        nv, lod = pg.nvalid, pc.lam_over_d(pg, tel)
        along, across = [], []
        for amp in (0.5, 1.0, 2.0):
            _, s = m.measure(pc.tilt_phase(pg, tel, geom, amp, axis)[None])
            sx, sy = s[0, :nv].mean(), s[0, nv:].mean()
            along.append(sx if axis == 1 else sy)
            across.append(sy if axis == 1 else sx)
        print("%s axis %d: mean slope / tilt at 0.5, 1, 2 lambda/D: %s" % (tag, axis, [a / (t * lod) for a, t in zip(along, (0.5, 1, 2))]))
        assert 0.9 <= along[1] / lod <= 1.3, tag
        assert abs(across[1]) <= 1e-9 * along[1], tag
        assert 0 < along[0] < along[1] < along[2], tag


def test_the_four_methods(golden):
    geom, sz, pg, tel, w = pc.build(golden, "tinyA")
    m = PyramidModel(pg, thresh=0.)
    ph = pc.smooth_phases(pg, tel, geom, 1, seed=3)
    img, _ = m.measure(ph)
    nv = pg.nvalid
    q = img[0][pg.validsubsx, pg.validsubsy].reshape(4, nv)
    tot = q.sum(axis=0)
    rx, ry = (q[1] + q[3]) - (q[0] + q[2]), (q[1] + q[2]) - (q[0] + q[3])
    raw = {0: np.concatenate([rx, ry]) / tot.mean(), 2: np.concatenate([rx / tot, ry / tot])}
    for method in (0, 1, 2, 3):
        want = raw[method & 2]
        want = pg.s_scale * (np.sin(np.pi / 2 * want) if method & 1 else want)
        got = m.slopes(img[0], method)
        assert np.abs(got - want).max() <= 1e-12 * pg.s_scale, method
    s = [m.slopes(img[0], k) for k in range(4)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert np.abs(s[a] - s[b]).max() > 1e-4 * pg.s_scale, (a, b)
    m.set_ref(s[1])
    assert not m.slopes(img[0], 1).any()


def test_thresh_zeroes_a_dark_point(golden):
    geom, sz, pg, tel, w = pc.build(golden, "tinyA")
    m = PyramidModel(pg, method=2)
    img, _ = m.measure(pc.smooth_phases(pg, tel, geom, 1, seed=4))
    img = img[0].copy()
    nv = pg.nvalid
    dark = 7
    for j in range(4):
        img[pg.validsubsx[j * nv + dark], pg.validsubsy[j * nv + dark]] *= 1e-9
    tot = img[pg.validsubsx, pg.validsubsy].reshape(4, nv).sum(axis=0)
    m.thresh = float(np.sort(tot)[1] / 2)           # between the dark point and every other one
    for method in (2, 3):
        s = m.slopes(img, method)
        assert s[dark] == 0 and s[nv + dark] == 0
        assert np.count_nonzero(s[:nv]) == nv - 1
    m.thresh = float(2 * tot.mean())                # the global normaliser below thresh: everything is zero
    assert not m.slopes(img, 0).any() and not m.slopes(img, 1).any()


# ------------------------------------------------------------------------------------------------ 3. refusals, modulation
def test_refusals_by_name(golden):
    tel, w, ittime = pc.params_of(golden, "tinyA")
    geom = G.pupil_geometry(32, tel)
    for kw, word in ((dict(nPupils=3), "nPupils"), (dict(pyr_misalignments=np.zeros((4, 2))), "pyr_misalignments"),
                     (dict(type="pyrlr"), "pyrlr"), (dict(gsalt=90000.), "LGS"), (dict(nxsub=5), "pupdiam")):
        _, bad, _ = pc.params_of(golden, "tinyA", **kw)
        with pytest.raises(NotImplementedError, match=word):
            G.pyr_geometry(bad, G.pyr_sizes(bad, tel, geom.pupdiam), geom, tel, ittime)
    _, four, _ = pc.params_of(golden, "tinyA", nPupils=4)
    assert G.pyr_sizes(four, tel, geom.pupdiam).Nfft == 128
    _, bad, _ = pc.params_of(golden, "tinyA", fstop="hexagon")
    with pytest.raises(ValueError, match="fstop"):
        G.pyr_geometry(bad, G.pyr_sizes(bad, tel, geom.pupdiam), geom, tel, ittime)
    with pytest.raises(NotImplementedError, match="Shack-Hartmann"):       # the system builder is as it was
        ps = P.builtin("production_sh_10x10_2m")
        ps.p_wfss[0].type = "pyrhr"
        G.build_system(ps)
    with pytest.raises(ValueError, match="method"):
        PyramidModel(G.pyr_geometry(w, G.pyr_sizes(w, tel, geom.pupdiam), geom, tel, ittime), method=4)


def test_new_parameter_defaults():
    w, c = P.Param_wfs(), P.Param_centroider()
    assert (w.pyr_ampl, w.pyr_npts, w.pyr_pos, w.pyr_pup_sep, w.fssize, w.fstop, w.nPupils, w.pyr_misalignments) == \
        (0.0, 0, None, -1, 0.0, None, 0, None)
    assert c.method == 1 and c.thresh == 1.0e-4


def test_set_modulation_weights(golden):
    geom, sz, pg, tel, w = pc.build(golden, "tinyA")
    m = PyramidModel(pg)
    ph = pc.smooth_phases(pg, tel, geom, 1, seed=5)
    cx, cy = pg.pyr_cx[[1, 6, 11]], pg.pyr_cy[[1, 6, 11]]
    wts = np.array([0.5, 2.0, 1.25])
    m.set_modulation(cx, cy, wts)
    both, _ = m.measure(ph)
    singles = []
    for k in range(3):
        m.set_modulation(cx[k:k + 1], cy[k:k + 1], [1.0])
        singles.append(m.measure(ph)[0])
    want = sum(wk * s for wk, s in zip(wts, singles)) / wts.sum()
    assert np.abs(both - want).max() <= 1e-12 * want.max()
    m.set_modulation(cx, cy, 3 * wts)
    assert np.abs(m.measure(ph)[0] - both).max() <= 1e-12 * both.max()      # only the shares count
    for bad in ([1, -1, 1], [0, 0, 0], [1, np.nan, 1], [1, 1]):
        with pytest.raises(ValueError, match="weights|number of points"):
            m.set_modulation(cx, cy, bad)


def test_set_modulation_ampli_scaling(golden):
    tel, w, ittime = pc.params_of(golden, "tinyA")
    geom = G.pupil_geometry(32, tel)
    sen = PyramidSensor.from_geometry(geom, tel, w, P.Param_centroider(type="pyr", method=1), ittime, device="cpu")
    assert sen.s_scale == pytest.approx(pc.scalar(golden, "tinyA", "s_scale"), rel=1e-12)
    r3 = np.hypot(sen.cx, sen.cy)
    tilt = pc.tilt_phase(sen.pg, tel, geom, 0.5, 1)[None]
    s3 = sen.measure(tilt)[0, :sen.nvalid].mean()
    scale = sen.set_modulation_ampli(1.5)
    assert scale == pytest.approx(0.5 * pc.scalar(golden, "tinyA", "s_scale"), rel=1e-12) and sen.s_scale == scale
    assert np.allclose(np.hypot(sen.cx, sen.cy), 0.5 * r3, rtol=1e-12) and sen.cx.size == 16
    s15 = sen.measure(tilt)[0, :sen.nvalid].mean()
    # half the radius doubles the raw signal of a small tilt and halves the unit: the slope in arcsec keeps its unit
    # response (the band of the tilt test; with 16 points a radius much above 3 lambda / D samples the circle too thinly)
    lod = pc.lam_over_d(sen.pg, tel)
    print("slope / tilt at 3 lambda/D: %.4f, at 1.5 lambda/D: %.4f" % (s3 / (0.5 * lod), s15 / (0.5 * lod)))
    assert 0.9 <= s3 / (0.5 * lod) <= 1.3 and 0.9 <= s15 / (0.5 * lod) <= 1.3
    sen.set_modulation(sen.cx[:4], sen.cy[:4], [1, 2, 3, 4])
    assert sen.weights.tolist() == [1, 2, 3, 4] and sen.native.model.w.tolist() == [1, 2, 3, 4]
    with pytest.raises(RuntimeError, match="stand-alone"):
        sen.calibrate()
    with pytest.raises(RuntimeError, match="stand-alone"):
        sen.start()


def test_noise_rule_statistics():
    """pyr_noise (the NumPy statement of the device's draw rule): Poisson mean and variance on both branches, read-out
    noise on top, a fresh block per frame"""
    for lam in (3.0, 200.0):
        v = pyr_noise(np.full(40000, lam, dtype=np.float32), 0.0, seed=11, frame=5)
        assert abs(v.mean() - lam) < 5 * np.sqrt(lam / v.size) and abs(v.var() / lam - 1) < 0.05
        assert np.array_equal(v, np.round(v)) and v.min() >= 0
    z = np.zeros(40000, dtype=np.float32)
    r = pyr_noise(z, 2.5, seed=11, frame=5)
    assert abs(r.std() - 2.5) < 0.05 and abs(r.mean()) < 0.05
    assert not np.array_equal(r, pyr_noise(z, 2.5, seed=11, frame=6))
    assert np.array_equal(pyr_noise(z + 7, -1.0, 1, 1), z + 7)


# ------------------------------------------------------------------------------------------------ 4. host half
def test_host_check_builds_and_passes(tmp_path):
    """pyr_host_check.cpp under the address and undefined-behaviour sanitizers: the validators' refusals, the batch plan
    (every pair once, inside the budget) and the launch count; the Makefile's host_check target runs it too"""
    exe = str(tmp_path / "pyr_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "pyr_host_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "pyr_host_check: ok"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    line = [ln for ln in mk.splitlines() if "_host_check.cpp" in ln][0]
    assert " pyr " in line and "build/aomarl_pyr.o" in mk
