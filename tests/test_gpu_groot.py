"""The GROOT covariance model on the device (csrc/aomarl_groot.hip through ao_marl_amd/groot.py) against the float64
restatement (tests/groot_reference.py).

k_groot_form evaluates the structure functions and the tap sum in double and rounds once, so its bound is stated, not
measured:  |device - f64| <= ulp32(|value|) + 1e-12 sum_t |w_t F_t|  (the second term: 25 x the 16 ulp the OpenCL
specification allows a double pow, over a chain of about ten such operations).
The full covariances pass two fp32 products; their allowance is 4 x the error of the CPU statement with the same rounding
points (GrootModel(device="cpu", dtype=np.float32): the form rounded to float32, the products in NumPy float32), measured
by the test at run time -- the project's convention for fp32 kernels checked against float64.  Every
test prints the device's error beside the allowance."""
import ctypes as C

import numpy as np
import pytest

from tests import groot_reference as gr
from tests.test_groot import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cases():
    """name -> dict(c: the file, gpu / f32 / f64: the three models); built once, left unchanged"""
    from ao_marl_amd import groot
    out = {}
    with np.load(GOLDEN) as z:
        for n in ("A", "B"):
            c = gr.case(z, n)
            out[n] = dict(c=c, gpu=groot.GrootModel(c, device=DEV), f32=groot.GrootModel(c, dtype=np.float32),
                          f64=groot.GrootModel(c))
    return out


def _specs(m, kind):
    if kind == "cerr":
        return "act", [m.cerr_spec()[0]]
    if kind == "calias":
        return "sub", list(m.calias_specs(5))
    return "sub", list(m.dcmm_specs()[0])


@pytest.mark.parametrize("kind", ["cerr", "calias", "dcmm"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_form_kernel_against_float64(cases, name, kind):
    """45 / 69 actuators and 24 / 44 sub-apertures: no multiple of the 16 x 16 tile, more than one workgroup; case B takes
    both branches of both functions; 6 / 9 taps (Cerr), 27 (Calias, npts = 5), 12 / 18 (dCmm)"""
    from ao_marl_amd import groot
    m = cases[name]["gpu"]
    which, specs = _specs(m, kind)
    px, py = (m.xactu, m.yactu) if which == "act" else (m.xsub, m.ysub)
    for spec in specs:
        got = m._host(m.form(which, spec)).astype(np.float64)
        want, mag = gr.form_terms(px, py, groot.taps_of(spec))
        bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-12 * mag
        err = np.abs(got - want)
        worst = int(np.argmax(err - bound))
        print("%s %s %s: %d x %d, %d taps: max |device - f64| %.3e (largest value %.3e, sum |w F| %.3e); at the tightest "
              "element error %.3e, bound %.3e" % (name, kind, spec["model"], px.size, px.size, groot.taps_of(spec)["w"].shape[1],
                                                  err.max(), np.abs(want).max(), mag.max(), err.ravel()[worst],
                                                  bound.ravel()[worst]))
        assert got.shape == want.shape and np.abs(want).max() > 0
        assert (err <= bound).all(), (name, kind, spec["model"])


def _check(tag, got, f32, want):
    eg = float(np.abs(got - want).max() / np.abs(want).max())
    ec = float(np.abs(f32 - want).max() / np.abs(want).max())
    print("%s: device %.3e   CPU float32 %.3e   allowance %.3e   (relative to the largest value, %.3e)" %
          (tag, eg, ec, 4 * ec, np.abs(want).max()))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert eg <= 4 * ec, (tag, eg, ec)


@pytest.mark.parametrize("name", ["A", "B"])
def test_covariances_against_the_restatement(cases, name):
    k = cases[name]
    c, g, f = k["c"], k["gpu"], k["f32"]
    # the restatement with the float64 pzt2tt the product composes its factors from is not the yardstick: the reference's
    # float32 one is, as in the CPU tests
    _check(name + " cerr modal", g.cerr(), f.cerr(), gr.cerr(c))
    got = g.cerr(modal=False)
    _check(name + " cerr actuators", got, f.cerr(modal=False), gr.cerr(c, modal=False))
    assert not got[:-2, -2:].any() and not got[-2:, :-2].any()          # the tip-tilt block's cross terms stay zero
    _check(name + " calias slopes", g.calias(slopes_space=True), f.calias(slopes_space=True), gr.calias(c, slopes_space=True))
    _check(name + " calias actuators", g.calias(modal=False), f.calias(modal=False), gr.calias(c, modal=False))
    _check(name + " calias modal npts 5", g.calias(npts=5), f.calias(npts=5), gr.calias(c, npts=5))
    _check(name + " dcmm", g.dcmm(), f.dcmm(), gr.dcmm(c))


def test_batch_and_determinism(cases):
    """entry b of a batch of three atmospheres is the single call, bit for bit; a second run leaves the same bits"""
    k = cases["B"]
    g, c = k["gpu"], k["c"]
    speed = np.array([[0.4, 20., 15.], [5., 5., 5.], [12., 0.5, 30.]])
    theta = np.array([[0.1, -1.2, 3.0], [0., 0., 0.], [2., 1., -3.]])
    L0 = np.array([[2., 1e5, 25.], [25., 25., 25.], [1e5, 3., 50.]])
    r0 = np.array([0.12, 0.2, 0.08])
    for modal in (True, False):
        both = g.cerr(modal=modal, speed=speed, theta=theta, L0=L0, r0=r0)
        again = g.cerr(modal=modal, speed=speed, theta=theta, L0=L0, r0=r0)
        assert both.shape[0] == 3 and np.array_equal(both, again)
        for b in range(3):
            one = g.cerr(modal=modal, speed=speed[b], theta=theta[b], L0=L0[b], r0=r0[b])
            assert np.array_equal(one, both[b]), (modal, b)
    over = dict(speed=speed[2], theta=theta[2], L0=L0[2], r0=r0[2])
    _check("B batch entry 2 cerr modal", g.cerr(speed=speed, theta=theta, L0=L0, r0=r0)[2], k["f32"].cerr(**over),
           gr.cerr(c, **over))
    d2 = g.dcmm(ws=speed, wd=theta * 50.)
    assert np.array_equal(d2[1], g.dcmm(ws=speed[1], wd=theta[1] * 50.)) and np.array_equal(d2, g.dcmm(ws=speed, wd=theta * 50.))
    assert np.array_equal(g.calias(), g.calias())


def test_refusals_of_the_library(cases):
    import torch
    from ao_marl_amd import libaomarl as la
    g = cases["A"]["gpu"]
    lib = la.load()
    with pytest.raises(ValueError, match="batch of 17"):
        g.cerr(r0=np.full(17, 0.1))
    spec = g.cerr_spec()[0]
    out = torch.zeros(1, g.na, (g.na + 3) & ~3, dtype=torch.float32, device=DEV)
    px, py = g.pts["act"]
    w = np.ascontiguousarray(spec["w"])
    f = la.GrootFormDesc()
    f.model, f.batch, f.nlayers, f.npts, f.x0 = la.GROOT_CERR, 1, 2, 0, 0.25
    f.w = f.sx = f.sy = f.L0 = la.dptr(w)
    sm = la.raw_stream(g.tdev)
    for change, text in ((dict(model=7), "model = 7"), (dict(batch=17), "batch = 17"), (dict(nlayers=0), "nlayers = 0"),
                         (dict(x0=0.0), "x0 must be positive")):
        h = la.GrootFormDesc.from_buffer_copy(f)
        for a, v in change.items():
            setattr(h, a, v)
        with pytest.raises(la.AomarlError, match=text):
            la.check(lib.aomarl_groot_form(g.ptr, C.byref(h), px.data_ptr(), py.data_ptr(), g.na, out.data_ptr(), out.shape[2],
                                           0, sm))
    with pytest.raises(la.AomarlError, match="n = %d points" % (g.na + 1)):
        la.check(lib.aomarl_groot_form(g.ptr, C.byref(f), px.data_ptr(), py.data_ptr(), g.na + 1, out.data_ptr(), 64, 0, sm))
    with pytest.raises(la.AomarlError, match="ldo = 44"):
        la.check(lib.aomarl_groot_form(g.ptr, C.byref(f), px.data_ptr(), py.data_ptr(), g.na, out.data_ptr(), 44, 0, sm))
    G = g.Gd["cerr_modal_pzt"]
    with pytest.raises(la.AomarlError, match="ldg = 45"):
        la.check(lib.aomarl_groot_sandwich(g.ptr, G.data_ptr(), 45, g.nm, out.data_ptr(), out.shape[2], g.na, out.data_ptr(),
                                           out.shape[2], 0, sm))
    with pytest.raises(la.AomarlError, match="m = %d rows" % (g.nactu + 1)):
        la.check(lib.aomarl_groot_sandwich(g.ptr, G.data_ptr(), G.shape[1], g.nactu + 1, out.data_ptr(), out.shape[2], g.na,
                                           out.data_ptr(), out.shape[2], 0, sm))
    d = la.GrootDesc()
    d.n_max, d.batch_max = 0, 1
    ptr = C.c_void_p()
    with pytest.raises(la.AomarlError, match="n_max = 0"):
        la.check(lib.aomarl_groot_create(C.byref(d), C.byref(ptr)))
    assert not ptr.value
    torch.cuda.synchronize()
    assert not out.any()                                                 # nothing was launched by a refused call


def test_10x10_end_to_end(tmp_path):
    """VecAoEnv -> VecRoket (30 frames, kept histories) -> GrootModel on the device, against the restatement on the saved
    file: 88 actuators, 87 modes, 64 sub-apertures.

    The model PSF has no golden from the reference: compute_PSF needs COMPASS's native Gamora, which does not exist here.
    It is pinned as the composition of pinned parts instead: Cee = Cerr + Cn + Calias of the restatement (pinned to the
    reference by tests/test_groot.py), the Vii reconstruction of tests/psf_rec_reference.py (pinned to the reference's
    psf_rec_vii_cpu by tests/test_psf_rec.py), and the fitting OTF (pinned by tests/test_groot.py), multiplied as
    compute_PSF multiplies them (:476-477)."""
    from ao_marl_amd import groot, roket
    from ao_marl_amd.env import VecAoEnv
    from tests import psf_rec_reference as pr
    env = VecAoEnv("production_sh_10x10_2m", 2, geo=True, frame_pipeline=False)
    rk = roket.VecRoket(env, 30, 5, keep_envs=(0, 1))
    rk.run(verbose=False)
    g = groot.GrootModel(rk)
    assert g.device.startswith("cuda") and (g.na, g.nm, g.nsub) == (88, 87, 64)
    path = str(tmp_path / "budget.npz")
    rk.save(path)
    with np.load(path) as z:
        f = {k: z[k] for k in z.files}
    assert f["Nact"].shape == (88, 88) and float(f["_Param_controller__gain"]) == float(env.supervisor.gain)
    f32 = groot.GrootModel(path, dtype=np.float32)
    f64 = groot.GrootModel(path)
    assert abs(f64.pitch - 0.2) < 1e-12 and abs(f64.dsub - 0.2) < 1e-12
    _check("10x10 cerr", g.cerr(), f32.cerr(), gr.cerr(f))
    _check("10x10 calias", g.calias(), f32.calias(), gr.calias(f))
    # a sweep over four atmospheres in one call, against single restatements
    speed = np.array([[5.], [10.], [20.], [40.]])
    sweep = g.cerr(speed=speed, r0=np.array([0.1, 0.16, 0.2, 0.3]))
    assert sweep.shape == (4, 87, 87)
    _check("10x10 cerr, entry 3 of a sweep", sweep[3], f32.cerr(speed=speed[3], r0=0.3), gr.cerr(f, speed=speed[3], r0=0.3))
    # the model PSF of environment 1
    got = g.psf(env=1)
    c32 = f32.psf(env=1)
    N = np.asarray(f["noise"][1], dtype=np.float64)
    P = np.asarray(f["P"], dtype=np.float64)
    cee = gr.cerr(f) + P.dot(N.dot(N.T) / N.shape[1]).dot(P.T) + gr.calias(f)
    csr = (f["IF.data"], f["IF.indices"], f["IF.indptr"])
    ref = pr.vii_f64(f["spup"], csr, f["TT"], f["Btt"], cee, float(f["tar_lambda"][0]))
    otf_fit, _ = f64.otf_fitting(ref["otftel"])
    want = pr.psf_with(otf_fit * ref["otftel"], ref["otf2"], int(np.count_nonzero(f["spup"])))
    eg = float(np.abs(got["psf"] - want).max() / want.max())
    ec = float(np.abs(c32["psf"] - want).max() / want.max())
    print("10x10 model psf/peak: device %.3e   CPU float32 %.3e   allowance %.3e   (model Strehl %.4f, without the fitting "
          "OTF %.4f)" % (eg, ec, 4 * ec, want.max(), ref["psf"].max()))
    assert 0.0 < want.max() < 1.0 and got["psf"].shape == want.shape
    assert eg <= 4 * ec
