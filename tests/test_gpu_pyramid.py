"""Pyramid sensor on the device (csrc/aomarl_pyr.hip through ao_marl_amd/pyramid.py) against the float64 model
(pyramid.PyramidModel), its determinism, its noise against the oracle's draw rule, its sign and unit against the
Shack-Hartmann sensor of the 10x10 system, the closed loop and the environment.

Tolerances of the kernel tests: the yardstick is float64; the allowance is 4 x the error of the SAME model in float32
on the CPU (PyramidModel(dtype=np.float32): NumPy complex64 transforms on the same inputs), measured by the test at run
time -- the project's convention for fp32 kernels checked against float64 (tests/test_gpu_psf_rec.py).  The image is
compared relative to its peak, the slopes in arcsec.  Every test prints the device's error beside the CPU's."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import geometry as G, params as P  # noqa: E402
from ao_marl_amd.pyramid import NativePyramid, PyramidModel, PyramidSensor  # noqa: E402
from tests import pyramid_cases as pc  # noqa: E402

DEV = "cuda:0"
NAME = "production_sh_10x10_2m"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
NENV = 4


@pytest.fixture(scope="module")
def golden():
    with np.load(pc.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case(golden, name):
    """(pg, phases [3][n][n], cx, cy, weights, pixel_filter)"""
    if name == "A":             # Nfft 128, n 36; 4 points (on the pyramid's edges), unequal weights
        geom, sz, pg, tel, w = pc.build(golden, "tinyA", pyr_npts=4)
        wts = np.array([1.0, 0.25, 2.0, 0.5])
    elif name in ("B", "Bnf"):  # Nfft 256, n 52 (no multiple of a wave or of 16), square stop, 5 points
        geom, sz, pg, tel, w = pc.build(golden, "tinyB", pyr_npts=5)
        wts = np.ones(5)
        assert pg.n == 52 and str(golden["tinyB_fstop"]) == "square"
    else:                       # Nfft 512, n 164: the 10x10 system at nxsub 20, 16 points
        geom, sz, pg, tel, w = pc.build(golden, "s10_20")
        wts = np.ones(16)
        assert (pg.Nfft, pg.n, pg.pyr_cx.size) == (512, 164, 16)
    return pg, pc.smooth_phases(pg, tel, geom, 3, seed=ord(name[0])), pg.pyr_cx, pg.pyr_cy, wts, name != "Bnf"


@pytest.fixture(scope="module")
def references(golden):
    """name -> (case, float64 images, float32 images): computed once, left unchanged"""
    out = {}
    for name in ("A", "B", "Bnf", "C"):
        c = _case(golden, name)
        pg, ph, cx, cy, wts, pf = c
        res = []
        for dt in (np.float64, np.float32):
            m = PyramidModel(pg, thresh=1e-4, pixel_filter=pf, dtype=dt)
            m.set_modulation(cx, cy, wts)
            res.append((m, m.measure(ph.astype(np.float32))[0]))
        out[name] = (c, res[0], res[1])
    return out


def _native(c, nenv=3):
    pg, ph, cx, cy, wts, pf = c
    nat = NativePyramid(pg, nenv, thresh=1e-4, pixel_filter=pf, device=DEV)
    nat.set_modulation(cx, cy, wts, pg.s_scale)
    return nat, torch.as_tensor(ph.astype(np.float32), device=DEV).contiguous()


@pytest.mark.parametrize("name", ["A", "B", "Bnf", "C"])
def test_native_against_float64(references, name):
    """Nfft 128 / 256 / 512: three LDS depths of the column pass; n = 36, 52, 164; 4 / 5 / 16 points (whole
    environments per batch); the pixel filter on and off; all four methods"""
    c, (m64, i64), (m32, i32) = references[name]
    pg = c[0]
    nat, ph = _native(c)
    peak = i64.max()
    for method in (0, 1, 2, 3):
        nat.measure(ph, method=method)
        img, sl = nat.image.cpu().numpy().astype(np.float64), nat.slopes.cpu().numpy().astype(np.float64)
        s64 = np.stack([m64.slopes(i, method) for i in i64])
        s32 = np.stack([m32.slopes(i, method) for i in i32]).astype(np.float64)
        eg_i, ec_i = np.abs(img - i64).max() / peak, np.abs(i32 - i64).max() / peak
        eg_s, ec_s = np.abs(sl - s64).max(), np.abs(s32 - s64).max()
        print("case %s method %d  image/peak: device %.3e  CPU float32 %.3e   slopes [arcsec]: device %.3e  CPU float32 "
              "%.3e  (largest slope %.3e)" % (name, method, eg_i, ec_i, eg_s, ec_s, np.abs(s64).max()))
        assert eg_i <= 4 * ec_i, (name, method, eg_i, ec_i)
        assert eg_s <= 4 * ec_s, (name, method, eg_s, ec_s)
    assert np.abs(s64).max() > 0.05 * pg.s_scale and img.shape == (3, pg.Nfft // pg.nrebin, pg.Nfft // pg.nrebin)


def test_points_in_several_batches(references):
    """the 40x40 shape holds two pairs a batch: an environment's points then come in several batches and the image is
    accumulated across launches.  The same path at Nfft 128 with a budget of one pair (200 KiB): the bits of the
    default plan, where all points of all environments are one batch"""
    c = references["A"][0]
    nat, ph = _native(c)
    nat.measure(ph, method=1)
    img, sl = nat.image.clone(), nat.slopes.clone()
    pg, _, cx, cy, wts, pf = c
    one = NativePyramid(pg, 3, thresh=1e-4, pixel_filter=pf, device=DEV, batch_kib=200)
    one.set_modulation(cx, cy, wts, pg.s_scale)
    one.measure(ph, method=1)
    assert torch.equal(one.image, img) and torch.equal(one.slopes, sl) and img.abs().max() > 0


def test_determinism(references):
    """three environments in one call against 1 + 2, and a second run: the same bits, image and slopes"""
    c = references["B"][0]
    nat, ph = _native(c)
    nat.measure(ph, method=1)
    img, sl = nat.image.clone(), nat.slopes.clone()
    nat.image.zero_(), nat.slopes.zero_()
    nat.measure(ph, method=1, env_begin=0, env_count=1)
    nat.measure(ph, method=1, env_begin=1, env_count=2)
    assert torch.equal(nat.image, img) and torch.equal(nat.slopes, sl)
    nat2, _ = _native(c)
    nat2.measure(ph, method=1)
    assert torch.equal(nat2.image, img) and torch.equal(nat2.slopes, sl)
    assert img.abs().max() > 0 and sl.abs().max() > 0


def test_noise_against_the_oracle(golden):
    """the device's noisy image against the oracle's aoref_sh_noise applied to the device's own noise-free image
    (nvalid = 1, npix2 = pixel count, same seed and frame): only the draw rule is under test.  Magnitude 9 puts the
    pixels on both branches of the Poisson draw (means below and above 30)."""
    from oracle import aoref
    geom, sz, pg, tel, w = pc.build(golden, "tinyB", gsmag=9., noise=3.0)
    nat = NativePyramid(pg, 3, thresh=1e-4, device=DEV)
    nat.set_modulation(pg.pyr_cx, pg.pyr_cy, np.ones(pg.pyr_cx.size), pg.s_scale)
    ph = torch.as_tensor(pc.smooth_phases(pg, tel, geom, 3, seed=9).astype(np.float32), device=DEV)
    seeds = torch.tensor([7, 8, 4000000000 - (1 << 32)], dtype=torch.int32, device=DEV)
    frame = torch.tensor([0, 5, 41], dtype=torch.int32, device=DEV)
    nat.measure(ph, method=1)
    clean = nat.image.cpu().numpy()
    assert clean.max() > 30 and (clean < 30).mean() > 0.3
    nat.measure(ph, method=1, noise=True, seeds=seeds, frame=frame)
    noisy = nat.image.cpu().numpy()
    assert frame.cpu().tolist() == [1, 6, 42]
    L = aoref.lib()
    for e, (sd, fr) in enumerate(((7, 0), (8, 5), (4000000000, 41))):
        want = clean[e].reshape(-1).copy()
        L.aoref_sh_noise(want, 1, want.size, 3.0, sd, fr)
        d = np.abs(noisy[e].reshape(-1) - want)
        print("environment %d: share of pixels that differ %.2e, largest difference %.3f" % (e, (d > 1e-3).mean(), d.max()))
        assert (d > 1e-3).mean() < 2e-4, (d > 1e-3).mean()
        assert d.max() <= 1.0 + 1e-3
    assert (noisy < 0).any() and np.abs(noisy - clean).max() > 3
    nat.measure(ph, method=1)                               # without the flag: no draw, the counter stays
    assert np.array_equal(nat.image.cpu().numpy(), clean) and frame.cpu().tolist() == [1, 6, 42]


# ------------------------------------------------------------------------------------------------ the 10x10 system
@pytest.fixture(scope="module")
def loop():
    """(supervisor, calibrated sensor at nxsub 20) of the 10x10 system, 4 environments"""
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(P.builtin(NAME), RL, NENV)
    pyr = PyramidSensor(sup, nxsub=20)
    assert (pyr.pg.Nfft, pyr.pg.nrebin, pyr.pg.n) == (512, 8, 164)
    cmat = pyr.calibrate()
    print("calibration: doubled-push deviation %.3e (pushes of 0.01 um rms of phase)" % pyr.linearity)
    assert cmat.shape == (sup.s.nactu, pyr.nslope) and np.isfinite(cmat).all()
    return sup, pyr


def test_calibration_is_linear(loop):
    sup, pyr = loop
    print("doubled-push deviation %.3e" % pyr.linearity)
    assert pyr.linearity < 0.10


def test_cross_sensor_sign_and_unit(loop):
    """a tip, then a tilt command of 0.5 lambda / D on the TT mirror, through the simulator: both sensors in arcsec"""
    sup, pyr = loop
    sim, na, nv, nsh = sup.sim, sup.s.nactu, pyr.nvalid, sup.s.nvalid
    lod = pyr.pg.Lambda * 1e-6 / sup.config.p_tel.diam * G.RAD2ARCSEC
    unit = np.zeros((2, na), dtype=np.float32)
    unit[0, na - 2] = unit[1, na - 1] = 1.0
    sh1 = sim.dm_response(unit, geometric=False).astype(np.float64)
    for k in (0, 1):
        mx, my = sh1[k, :nsh].mean(), sh1[k, nsh:].mean()
        main = mx if abs(mx) > abs(my) else my
        cmd = unit[k:k + 1] * np.float32(0.5 * lod / abs(main))
        sh = sim.dm_response(cmd, geometric=False).astype(np.float64)[0]
        py = pyr._response(cmd)[0]
        s_sh = np.array([sh[:nsh].mean(), sh[nsh:].mean()])
        s_py = np.array([py[:nv].mean(), py[nv:].mean()])
        a = int(np.argmax(np.abs(s_sh)))
        print("TT actuator %d: SH mean slopes (%.5f, %.5f), pyramid (%.5f, %.5f) arcsec; 0.5 lambda/D = %.5f; ratio %.4f"
              % (k, s_sh[0], s_sh[1], s_py[0], s_py[1], 0.5 * lod, s_py[a] / s_sh[a]))
        assert abs(abs(s_sh[a]) / (0.5 * lod) - 1) < 0.05
        assert np.sign(s_py[a]) == np.sign(s_sh[a])
        assert 0.85 <= s_py[a] / s_sh[a] <= 1.35
        assert abs(s_py[1 - a]) < 0.02 * abs(s_py[a])
    sim.comp_dm_shape()


def _run(sup, nframes, lo):
    """bare loop: (mean science-path phase variance over frames lo.., long-exposure Strehl, commands of every frame)"""
    sup.reset()
    var = torch.zeros(sup.sim.nenv, dtype=torch.float64, device=DEV)
    coms = []
    sup.next_part_one()
    for t in range(nframes):
        sup.next_part_two(None, linear_control=True)
        if t >= lo:
            var += sup.get_strehl()[:, 2].double()
        sup.next_part_one()
        coms.append(sup.get_command().clone())
    return float(var.mean() / (nframes - lo)), float(sup.get_strehl()[:, 1].mean()), coms


def test_closed_loop(loop):
    """10x10, 4 environments, nxsub 20, 300 frames, the configuration's gain"""
    sup, pyr = loop
    gain = sup.gain
    assert gain == pytest.approx(0.7)
    sup.set_gain(0.0)
    v_open, sr_open, _ = _run(sup, 300, 100)
    sup.set_gain(gain)
    v_sh, sr_sh, _ = _run(sup, 300, 100)
    pyr.start()
    try:
        assert sup.get_slopes() is pyr.slopes
        v_pyr, sr_pyr, coms = _run(sup, 300, 100)
    finally:
        pyr.stop()
    assert sup.pyramid is None and sup.get_slopes() is not pyr.slopes
    print("doubled-push deviation %.3e" % pyr.linearity)
    print("phase variance, frames 100-300: open loop %.4f, SH integrator %.4f, pyramid integrator %.4f"
          % (v_open, v_sh, v_pyr))
    print("long-exposure Strehl: open loop %.4f, SH integrator %.4f, pyramid integrator %.4f" % (sr_open, sr_sh, sr_pyr))
    assert pyr.linearity < 0.10
    assert v_pyr < 0.25 * v_open
    assert all(torch.isfinite(c).all() for c in coms[-3:])


def test_start_refusals(loop):
    from ao_marl_amd.env import VecRlSupervisor
    sup, pyr = loop
    fresh = PyramidSensor(sup, nxsub=20)
    with pytest.raises(RuntimeError, match="calibrate"):
        fresh.start()
    sup.set_gain(np.full(NENV, 0.5, dtype=np.float32))
    with pytest.raises(RuntimeError, match="per-environment gains"):
        pyr.start()
    sup.set_gain(0.7)
    sup.set_modal_gains(np.ones(sup.nmodes, dtype=np.float32))
    with pytest.raises(RuntimeError, match="modal gains"):
        pyr.start()
    sup.set_modal_gains(None)
    for attr, word in (("online_modal_gains", "on-line modal-gain optimiser"), ("modal_predictor", "modal predictor"),
                       ("autoencoder", "denoiser"), ("geo", "GEO twin")):
        keep = getattr(sup, attr, None)
        setattr(sup, attr, object())
        try:
            with pytest.raises(RuntimeError, match=word):
                pyr.start()
        finally:
            setattr(sup, attr, keep)
    sup.reset_prefetch = "same"
    with pytest.raises(RuntimeError, match="prefetched reset"):
        pyr.start()
    sup.reset_prefetch = None
    sup.pure_delay_0 = True
    with pytest.raises(NotImplementedError, match="modification_online"):
        pyr.start()
    sup.pure_delay_0 = False
    sup.sim._twin = object()
    try:
        with pytest.raises(RuntimeError, match="frame pipeline"):
            pyr.start()
    finally:
        sup.sim._twin = None
    pyr.start()
    with pytest.raises(RuntimeError, match="already"):
        PyramidSensor.start(pyr)
    with pytest.raises(RuntimeError, match="stop"):
        pyr.calibrate()
    pyr.stop()
    assert sup.pyramid is None


def _env():
    from ao_marl_amd.env import VecAoEnv
    return VecAoEnv(P.builtin(NAME), NENV, RL, n_agents_modal=1, frame_pipeline=False)


def test_environment(loop):
    """VecAoEnv with the sensor attached, default state layout: the call-by-call path, the bare loop's commands"""
    sup, pyr = loop
    env, twin = _env(), _env()
    esup = env.supervisor
    mine = PyramidSensor(esup, nxsub=20)
    mine.cmat, mine.linearity = pyr.cmat, pyr.linearity          # the same system: the calibration carries over
    mine.set_ref(pyr.ref)
    s_twin = twin.reset()
    zero = torch.zeros(NENV, env.action_dim, device=DEV)
    mine.start()
    assert not env._native_step_ok(False)
    s = env.reset()
    assert s.shape == s_twin.shape
    # the bare supervisor loop of the closed-loop test on the same seeds
    pyr.start()
    try:
        sup.reset()
        sup.next_part_one()
        for t in range(20):
            s, r, _, _ = env.step(zero, linear_control=True)
            sup.next_part_two(None, linear_control=True)
            sup.next_part_one()
            assert s.shape == s_twin.shape and torch.isfinite(s).all()
            assert torch.equal(esup.get_command(), sup.get_command()), t
            assert torch.equal(esup.get_slopes(), sup.get_slopes()), t
    finally:
        pyr.stop()
    assert esup.get_command().abs().max() > 0
    s, r, _, _ = env.step(zero)                                  # the agents' (zero) action on the call-by-call path
    assert s.shape == s_twin.shape and torch.isfinite(s).all() and r.shape[0] == NENV and torch.isfinite(r).all()
    mine.stop()
    # after stop(): one step equals a never-attached twin bit for bit
    sa, sb = env.reset(), twin.reset()
    assert torch.equal(sa, sb)
    act = 0.1 * torch.randn(NENV, env.action_dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    (sa, ra, _, _), (sb, rb, _, _) = env.step(act), twin.step(act)
    assert torch.equal(sa, sb) and torch.equal(ra, rb)
    assert torch.equal(esup.get_command(), twin.supervisor.get_command())
