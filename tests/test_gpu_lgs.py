"""Laser guide star on the device (csrc/aomarl_lgs.hip through ao_marl_amd/lgs.py) against the float64 model
(lgs.LgsModel, lgs.cone_trace_model), its determinism, its noise against the oracle's draw rule, the calibration, the
closed loop and the environment.

Tolerances of the kernel tests: the yardstick is float64; the allowance is 4 x the error of the SAME model in float32 on
the CPU (LgsModel(dtype=np.float32), cone_trace_model(dtype=np.float32)) on the same inputs, measured by the test at run
time -- the project's convention for fp32 kernels checked against float64 (tests/test_gpu_pyramid.py).  The image is
compared relative to its peak, the slopes in arcsec, the phase in microns.  Every test prints the device's error beside
the CPU's.  The device holds the kernels in float32: the models are handed the rounded numbers."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import lgs as L, params as P  # noqa: E402
from tests import lgs_cases as lc  # noqa: E402

DEV = "cuda:0"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
NENV = 4


def _f32(K):
    return np.asarray(K, dtype=np.float32).astype(np.float64)


def _case(name):
    """(SimArrays, kernels rounded to float32, phases [3][n][n] float32: the last with three waves of tilt per
    sub-aperture, the spot three quarters of the way to the window's edge)"""
    pup = 80 if name == "small" else None
    _, _, s = lc.system_of(pupdiam=pup)
    if name == "impulse":
        K = L.impulse_kernels(s.nvalid, s.nfft)
    else:
        K = lc.kernels((0., 0.) if name == "centre" else (-3., -3.), pupdiam=pup)
    return s, _f32(K), lc.smooth_phases(s, 3, seed=ord(name[0]), waves_of_tilt=3.0).astype(np.float32)


@pytest.fixture(scope="module")
def references():
    """name -> (case, float64 (cube, slopes), float32 (cube, slopes)): computed once, left unchanged"""
    out = {}
    for name in ("centre", "side", "impulse", "small"):
        s, K, ph = c = _case(name)
        out[name] = (c, L.LgsModel(s, K, noise=-1).measure(ph), L.LgsModel(s, K, noise=-1, dtype=np.float32).measure(ph))
    return out


def _native(c, nenv=3, **kw):
    s, K, ph = c
    return L.NativeLgs(s, nenv, K, device=DEV, **kw), torch.as_tensor(ph, device=DEV).contiguous()


# ------------------------------------------------------------------------------------------------ 1. device / float64
@pytest.mark.parametrize("name", ["centre", "side", "impulse", "small"])
def test_native_against_float64(references, name):
    """nvalid = 64 at pdiam 16 / N 64 (centre launch, side launch (-3, -3), the impulse) and nvalid = 72 at pdiam 8 /
    N 32; three environments, the last with the spot near the window's edge"""
    c, (i64, s64), (i32, s32) = references[name]
    s = c[0]
    assert (s.pdiam, s.nfft, s.nvalid) == ((8, 32, 72) if name == "small" else (16, 64, 64))
    nat, ph = _native(c)
    nat.measure(ph)
    img, sl = nat.image.cpu().numpy().astype(np.float64), nat.slopes.cpu().numpy().astype(np.float64)
    peak = i64.max()
    eg_i, ec_i = np.abs(img - i64).max() / peak, np.abs(i32 - i64).max() / peak
    eg_s, ec_s = np.abs(sl - s64).max(), np.abs(s32.astype(np.float64) - s64).max()
    print("case %s  image/peak: device %.3e  CPU float32 %.3e   slopes [arcsec]: device %.3e  CPU float32 %.3e  (largest "
          "slope %.3f)" % (name, eg_i, ec_i, eg_s, ec_s, np.abs(s64).max()))
    # (the tilted phase puts the spot well out towards the window's edge, 2.06 arcsec from its centre; at N = 32 the
    # window is the whole image and the centre of gravity of the wrapped wings reads less)
    assert np.abs(s64[2]).max() > 0.4 * (0.5 * s.npix * s.cog_scale) and img.shape == (3, s.nvalid, s.npix * s.npix)
    assert eg_i <= 4 * ec_i, (name, eg_i, ec_i)
    assert eg_s <= 4 * ec_s, (name, eg_s, ec_s)
    nat.slopes.zero_()
    keep = nat.image.clone()
    nat.measure(ph, write_cube=False)                       # the slopes alone: the same bits, the cube untouched
    assert torch.equal(nat.image, keep) and np.array_equal(nat.slopes.cpu().numpy().astype(np.float64), sl)


def test_create_starts_with_the_impulse(references):
    """aomarl_lgs_create's kernels are the impulse: set_kernels with the impulse changes no bit"""
    c = references["impulse"][0]
    nat, ph = _native(c)
    nat.measure(ph)
    img, sl = nat.image.clone(), nat.slopes.clone()
    fresh = L.NativeLgs(c[0], 3, None, device=DEV)
    fresh.measure(ph)
    assert torch.equal(fresh.image, img) and torch.equal(fresh.slopes, sl)
    ref = np.linspace(-1, 1, 2 * c[0].nvalid).astype(np.float32)
    nat.set_ref(ref)
    nat.measure(ph)
    assert np.abs(nat.slopes.cpu().numpy() - (sl.cpu().numpy() - ref[None])).max() <= 1e-6
    with pytest.raises(Exception, match="not negative"):
        nat.set_kernels(-np.abs(c[1]))
    with pytest.raises(Exception, match="environments"):
        nat.measure(ph, env_begin=2, env_count=2)


# ------------------------------------------------------------------------------------------------ 2. the cone trace
@pytest.mark.parametrize("alts", [(8000.,), (0., 4500., 14000.)])
def test_trace_against_the_model(alts):
    from ao_marl_amd.sim import HipSim
    _, sysm, s = lc.system_of(list(alts))
    sim = HipSim(s, nenv=3, device=DEV, keep_phase=True)
    sim.reset([11, 12, 13])
    for _ in range(3):
        sim.move_atmos()
    rng = np.random.default_rng(2)
    sim.comp_dm_shape(torch.as_tensor(0.05 * rng.normal(size=(3, s.nactu)).astype(np.float32), device=DEV))
    nat = L.NativeLgs(s, 3, L.impulse_kernels(s.nvalid, s.nfft), device=DEV)
    # delta = 1: today's trace, bit for bit, mirrors included
    sim.raytrace_wfs(atm=True, dms=True, reset=True)
    plain = sim.t["wfs_phase"].clone()
    nat.trace(sim, np.ones(len(alts)))
    assert torch.equal(sim.t["wfs_phase"], plain) and plain.abs().max() > 0
    # the cone: the atmosphere alone against the model, then the mirrors on top as today's trace adds them
    deltas = L.cone_deltas(sysm.atm.alt, 90e3)
    nat.trace(sim, deltas, atm=True, dms=False)
    got = sim.t["wfs_phase"].cpu().numpy().astype(np.float64)
    scr = [sim.screen(l).cpu().numpy() for l in range(len(alts))]
    eg = ec = 0.0
    for e in range(3):
        layers = [a[e] for a in scr]
        m64 = L.cone_trace_model(layers, s.wfs_atm_off, deltas, s.n)
        m32 = L.cone_trace_model(layers, s.wfs_atm_off, deltas, s.n, dtype=np.float32).astype(np.float64)
        eg, ec = max(eg, np.abs(got[e] - m64).max()), max(ec, np.abs(m32 - m64).max())
    print("layers at %r m, delta %r: phase [um]: device %.3e  CPU float32 %.3e  (largest phase %.3f)"
          % (alts, np.round(deltas, 4).tolist(), eg, ec, np.abs(got).max()))
    assert eg <= 4 * ec and np.abs(got - plain.cpu().numpy()).max() > 1e-3
    nat.trace(sim, deltas, atm=True, dms=True)
    both = sim.t["wfs_phase"].clone()
    sim.raytrace_wfs(atm=False, dms=True, reset=True)
    dm_only = sim.t["wfs_phase"].cpu().numpy().astype(np.float64)
    assert np.abs(both.cpu().numpy() - (got + dm_only)).max() <= 4 * ec + 1e-6 * np.abs(got).max()
    with pytest.raises(Exception, match="dm1"):
        nat.trace(sim, np.full(len(alts), 2.5))
    with pytest.raises(Exception, match="layers"):
        nat.trace(sim, np.ones(len(alts) + 1))


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_determinism(references):
    """three environments in one call against 1 + 2, and a second object: the same bits, cube and slopes"""
    c = references["side"][0]
    nat, ph = _native(c)
    nat.measure(ph)
    img, sl = nat.image.clone(), nat.slopes.clone()
    nat.image.zero_(), nat.slopes.zero_()
    nat.measure(ph, env_begin=0, env_count=1)
    nat.measure(ph, env_begin=1, env_count=2)
    assert torch.equal(nat.image, img) and torch.equal(nat.slopes, sl)
    nat2, _ = _native(c)
    nat2.measure(ph)
    assert torch.equal(nat2.image, img) and torch.equal(nat2.slopes, sl)
    assert img.abs().max() > 0 and sl.abs().max() > 0


# ------------------------------------------------------------------------------------------------ 4. noise
def test_noise_against_the_oracle(references):
    """the device's noisy cube against the oracle's aoref_sh_noise applied to the device's own noise-free cube (same
    seed and frame): only the draw rule is under test.  The pixels lie on both branches of the Poisson draw."""
    from oracle import aoref
    c = references["side"][0]
    s = c[0]
    nat, ph = _native(c, noise=3.0)
    seeds = torch.tensor([7, 8, 4000000000 - (1 << 32)], dtype=torch.int32, device=DEV)
    frame = torch.tensor([0, 5, 41], dtype=torch.int32, device=DEV)
    nat.measure(ph)
    clean, clean_sl = nat.image.cpu().numpy(), nat.slopes.clone()
    assert clean.max() > 30 and (clean < 30).mean() > 0.3
    nat.measure(ph, noise=True, seeds=seeds, frame=frame)
    noisy = nat.image.cpu().numpy()
    assert frame.cpu().tolist() == [1, 6, 42]               # the counters advance as the Shack-Hartmann's do
    lib = aoref.lib()
    for e, (sd, fr) in enumerate(((7, 0), (8, 5), (4000000000, 41))):
        want = clean[e].reshape(-1).copy()
        lib.aoref_sh_noise(want, s.nvalid, s.npix * s.npix, 3.0, sd, fr)
        d = np.abs(noisy[e].reshape(-1) - want)
        print("environment %d: share of pixels that differ %.2e, largest difference %.3f" % (e, (d > 1e-3).mean(), d.max()))
        assert (d > 1e-3).mean() < 2e-4, (d > 1e-3).mean()
        assert d.max() <= 1.0 + 1e-3
    assert (noisy < 0).any() and np.abs(noisy - clean).max() > 3 and not torch.equal(nat.slopes, clean_sl)
    nat.measure(ph)                                         # without the flag: no draw, the counter stays
    assert np.array_equal(nat.image.cpu().numpy(), clean) and frame.cpu().tolist() == [1, 6, 42]


# ------------------------------------------------------------------------------------------------ the 10x10 system
@pytest.fixture(scope="module")
def loop():
    """(supervisor, calibrated centre-launch sensor) of the 10x10 system, 4 environments"""
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(P.builtin(lc.CONFIG), RL, NENV)
    sen = L.LgsSensor(sup, gsalt=90e3, llt=(0., 0.))
    cmat = sen.calibrate()
    print("calibration: doubled-push deviation %.3e (pushes of 0.01 um rms of phase)" % sen.linearity)
    assert cmat.shape == (sup.s.nactu, sen.nslope) and np.isfinite(cmat).all()
    return sup, sen


# ------------------------------------------------------------------------------------------------ 5. calibration
def test_calibration_and_sign(loop):
    """linearity; cmat_lgs . imat is the projector onto the unfiltered modes; with the impulse kernel (and no layer
    above the ground: delta = 1) the sensor is the Shack-Hartmann: the same slopes on the device (1e-4 arcsec, the
    project's parity figure), and the command matrix built as the supervisor's own is built -- push and pull of
    push4imat per actuator, cmat_with_btt -- equals the supervisor's within 4 x the distance of the float32 model's
    matrix from the float64 model's on the same pushed phases."""
    from ao_marl_amd import modal
    sup, sen = loop
    sim, s = sup.sim, sup.s
    assert sen.linearity < 0.05
    m2v, v2m = np.asarray(sup.modes2volts, dtype=np.float64), np.asarray(sup.volts2modes, dtype=np.float64)
    nfilt = sup.n_reverse_filtered_from_cmat
    Bf = modal._btt_filtered(m2v, nfilt)
    D = sen.imat_modes @ v2m
    X = sen.cmat.astype(np.float64) @ D @ Bf
    print("cmat_lgs . imat . Bf against Bf: %.3e of its largest entry" % (np.abs(X - Bf).max() / np.abs(Bf).max()))
    assert np.abs(X - Bf).max() <= 1e-3 * np.abs(Bf).max()             # (a float32 command matrix)
    # the supervisor's own matrix is modal.imat_diffractive (push and pull of push4imat per actuator) through
    # cmat_with_btt: the same commands through the impulse-kernel sensor, the same two steps
    imp = L.LgsSensor(sup, kernels=L.impulse_kernels(s.nvalid, s.nfft))
    cmds = np.concatenate([modal._push_matrix(s, k, d.push4imat) for k, d in enumerate(s.dms)])
    push2 = np.float32(2) * np.abs(cmds).max(axis=1)
    plus, minus = imp._response(cmds), imp._response(-cmds)
    sh = sim.dm_response(np.concatenate([cmds, -cmds]), geometric=False).astype(np.float64)
    d_sh = np.abs(np.concatenate([plus, minus]) - sh).max()
    print("impulse kernel against the Shack-Hartmann on the device, %d pushes and pulls: slopes differ by %.3e arcsec"
          % (cmds.shape[0], d_sh))
    assert d_sh <= 1e-4
    # the pushed phases, as the device saw them (a pull is the push's phase negated, exactly)
    phases = np.zeros((cmds.shape[0], s.n, s.n), dtype=np.float32)
    for k0 in range(0, cmds.shape[0], NENV):
        nn = min(NENV, cmds.shape[0] - k0)
        sim.comp_dm_shape(imp._volts(cmds[k0:k0 + nn]))
        sim.raytrace_wfs(atm=False, dms=True, reset=True)
        phases[k0:k0 + nn] = sim.t["wfs_phase"][:nn].cpu().numpy()
    sim.comp_dm_shape(imp._volts(-cmds[:1]))
    sim.raytrace_wfs(atm=False, dms=True, reset=True)
    assert np.array_equal(sim.t["wfs_phase"][0].cpu().numpy(), -phases[0])
    sim.comp_dm_shape()
    K = _f32(imp.kernels)
    both = np.concatenate([phases, -phases])
    r64 = L.LgsModel(s, K, noise=-1).measure(both)[1]
    r32 = L.LgsModel(s, K, noise=-1, dtype=np.float32).measure(both)[1]
    na = cmds.shape[0]

    def cmat_of(p, m):
        imat = ((p - m).astype(np.float32).T / push2[None, :]).astype(np.float32)
        return modal.cmat_with_btt(imat, sup.modes2volts, nfilt).astype(np.float64)
    c_dev, c64, c32 = cmat_of(plus, minus), cmat_of(r64[:na], r64[na:]), cmat_of(r32[:na], r32[na:])
    sh_c = np.asarray(s.cmat, dtype=np.float64)
    assert sh_c.shape == c_dev.shape
    eg, ec, e_sh = np.abs(c_dev - c64).max(), np.abs(c32 - c64).max(), np.abs(c_dev - sh_c).max()
    print("command matrix, impulse kernel, per-actuator pushes: device %.3e  CPU float32 %.3e from the float64 model's; "
          "device from the supervisor's own %.3e  (largest entry %.3f)" % (eg, ec, e_sh, np.abs(sh_c).max()))
    assert eg <= 4 * ec
    assert e_sh <= 4 * ec


# ------------------------------------------------------------------------------------------------ 6. closed loop
def _run(sup, nframes, lo):
    """bare loop: (mean science-path phase variance over frames lo.., long-exposure Strehl, commands of the last frames)"""
    sup.reset()
    var = torch.zeros(sup.sim.nenv, dtype=torch.float64, device=DEV)
    coms = []
    sup.next_part_one()
    for t in range(nframes):
        sup.next_part_two(None, linear_control=True)
        if t >= lo:
            var += sup.get_strehl()[:, 2].double()
        sup.next_part_one()
        if t >= nframes - 3:
            coms.append(sup.get_command().clone())
    return float(var.mean() / (nframes - lo)), float(sup.get_strehl()[:, 1].mean()), coms


def test_closed_loop(loop):
    """10x10, 4 environments, 300 frames, the configuration's gain: the LGS loop's long-exposure residual phase variance
    below half the open loop's (a loop that does not close gives about 1 or more); the SH loop's value beside it"""
    sup, sen = loop
    gain = sup.gain
    sup.set_gain(0.0)
    v_open, sr_open, _ = _run(sup, 300, 100)
    sup.set_gain(gain)
    v_sh, sr_sh, _ = _run(sup, 300, 100)
    sen.start()
    try:
        assert sup.get_slopes() is sen.slopes
        v_lgs, sr_lgs, coms = _run(sup, 300, 100)
    finally:
        sen.stop()
    assert sup.lgs is None and sup.get_slopes() is not sen.slopes
    print("phase variance, frames 100-300: open loop %.4f, SH integrator %.4f, LGS integrator %.4f" % (v_open, v_sh, v_lgs))
    print("long-exposure Strehl: open loop %.4f, SH integrator %.4f, LGS integrator %.4f" % (sr_open, sr_sh, sr_lgs))
    assert v_lgs < 0.5 * v_open
    assert all(torch.isfinite(c).all() for c in coms)


def test_focal_anisoplanatism_is_visible():
    """one layer at 8000 m: the Strehl with the guide star at 90 km against one at 1e9 m (printed, not asserted)"""
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(lc.params([8000.]), RL, NENV)
    out = []
    for gsalt in (90e3, 1e9):
        sen = L.LgsSensor(sup, gsalt=gsalt, llt=(0., 0.))
        sen.calibrate()
        sen.start()
        try:
            out.append(_run(sup, 300, 100))
        finally:
            sen.stop()
    print("layer at 8000 m: guide star at 90 km: phase variance %.4f, Strehl %.4f;  at 1e9 m: %.4f, %.4f"
          % (out[0][0], out[0][1], out[1][0], out[1][1]))
    assert all(np.isfinite(v[:2]).all() for v in out)


# ------------------------------------------------------------------------------------------------ 7. start, stop, env
def test_start_refusals(loop):
    sup, sen = loop
    fresh = L.LgsSensor(sup)
    with pytest.raises(RuntimeError, match="calibrate"):
        fresh.start()
    sup.set_gain(np.full(NENV, 0.5, dtype=np.float32))
    with pytest.raises(RuntimeError, match="per-environment gains"):
        sen.start()
    sup.set_gain(0.7)
    sup.set_modal_gains(np.ones(sup.nmodes, dtype=np.float32))
    with pytest.raises(RuntimeError, match="modal gains"):
        sen.start()
    sup.set_modal_gains(None)
    for attr, word in (("online_modal_gains", "on-line modal-gain optimiser"), ("modal_predictor", "modal predictor"),
                       ("autoencoder", "denoiser"), ("geo", "GEO twin"), ("pyramid", "pyramid is attached"),
                       ("registration", "mis-registration")):
        keep = getattr(sup, attr, None)
        setattr(sup, attr, object())
        try:
            with pytest.raises(RuntimeError, match=word):
                sen.start()
        finally:
            setattr(sup, attr, keep)
    sup.reset_prefetch = "same"
    with pytest.raises(RuntimeError, match="prefetched reset"):
        sen.start()
    sup.reset_prefetch = None
    sup.pure_delay_0 = True
    with pytest.raises(NotImplementedError, match="modification_online"):
        sen.start()
    sup.pure_delay_0 = False
    sup.sim._twin = object()
    try:
        with pytest.raises(RuntimeError, match="frame pipeline"):
            sen.start()
    finally:
        sup.sim._twin = None
    sen.start()
    with pytest.raises(RuntimeError, match="already"):
        L.LgsSensor.start(sen)
    with pytest.raises(RuntimeError, match="stop"):
        sen.calibrate()
    from ao_marl_amd.pyramid import PyramidSensor
    pyr = PyramidSensor.__new__(PyramidSensor)
    pyr.sup, pyr.cmat = sup, sen.cmat
    with pytest.raises(RuntimeError, match="laser guide star is attached"):
        pyr.start()
    sen.stop()
    assert sup.lgs is None


def _env():
    from ao_marl_amd.env import VecAoEnv
    return VecAoEnv(P.builtin(lc.CONFIG), NENV, RL, n_agents_modal=1, frame_pipeline=False)


def test_environment(loop):
    """VecAoEnv with the sensor attached, default state layout: the call-by-call path, the bare loop's commands; after
    stop() the plain path's bits"""
    sup, sen = loop
    env, twin = _env(), _env()
    esup = env.supervisor
    mine = L.LgsSensor(esup, gsalt=90e3, llt=(0., 0.))
    mine.cmat, mine.linearity = sen.cmat, sen.linearity          # the same system: the calibration carries over
    mine.set_ref(sen.ref)
    s_twin = twin.reset()
    zero = torch.zeros(NENV, env.action_dim, device=DEV)
    mine.start()
    assert not env._native_step_ok(False)
    s = env.reset()
    assert s.shape == s_twin.shape
    sen.start()
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
        sen.stop()
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
