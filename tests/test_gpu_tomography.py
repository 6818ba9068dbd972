"""Laser tomography on the device (csrc/aomarl_tomo.hip through ao_marl_amd/tomography.py): k_tomo_trace against the
float64 model and against k_lgs_trace's bits, k_tomo_cov against the float64 statement, the sensor's calibration against
the host's, its refusals, the closed loop and the environment.

Tolerances: the trace is fp32 checked against float64 within 4 x the error of the SAME model in float32 on the CPU,
measured at run time (the convention of tests/test_gpu_lgs.py); the covariance is double checked against the float64
statement within 1e-12 of sum |w D| per element (the project's bound for double tap sums, tests/test_gpu_groot.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import lgs as L, tomography as T  # noqa: E402
from tests import tomo_cases as tc  # noqa: E402

DEV = "cuda:0"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
NENV = 4
SCI = [(0., 0., np.inf)]


# ------------------------------------------------------------------------------------------------ 1. the trace
@pytest.fixture(scope="module")
def traced():
    """(SimArrays, system, HipSim of 3 environments behind a reset, three moves and random mirror commands, its screens
    on the host, NativeTomo)"""
    from ao_marl_amd.sim import HipSim
    _, sysm, s = tc.system_of(tc.LAYERS_3)
    sim = HipSim(s, nenv=3, device=DEV, keep_phase=True)
    sim.reset([11, 12, 13])
    for _ in range(3):
        sim.move_atmos()
    rng = np.random.default_rng(2)
    sim.comp_dm_shape(torch.as_tensor(0.05 * rng.normal(size=(3, s.nactu)).astype(np.float32), device=DEV))
    scr = [sim.screen(l).cpu().numpy() for l in range(3)]
    return s, sysm, sim, scr, T.NativeTomo(DEV)


def _planes(sim, K):
    return torch.full((sim.nenv, K, sim.s.n, sim.s.n), 7.0, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("name", ["A", "B"])
def test_trace_against_the_model(traced, name):
    s, sysm, sim, scr, nat = traced
    stars = tc.STARS_A if name == "A" else tc.STARS_B
    off, dm1, delta = tc.assert_footprints_inside(sysm, stars)
    K = len(stars)
    pl = _planes(sim, K)
    nat.trace(sim, off, dm1, pl, atm=True, dms=False)
    got = pl.cpu().numpy().astype(np.float64)
    eg = ec = 0.0
    for e in range(3):
        layers = [a[e] for a in scr]
        m64 = T.tomo_trace_model(layers, off, delta, s.n)
        m32 = T.tomo_trace_model(layers, off, delta, s.n, dtype=np.float32).astype(np.float64)
        eg, ec = max(eg, np.abs(got[e] - m64).max()), max(ec, np.abs(m32 - m64).max())
    print("constellation %s: phase [um]: device %.3e  CPU float32 %.3e  (largest phase %.3f)" % (name, eg, ec, np.abs(got).max()))
    assert eg <= 4 * ec and np.abs(got[:, 1] - got[:, 0]).max() > 1e-3
    # the mirrors on top, as today's trace adds them: the same value on every plane
    both = _planes(sim, K)
    nat.trace(sim, off, dm1, both)
    sim.raytrace_wfs(atm=False, dms=True, reset=True)
    dm_only = sim.t["wfs_phase"].cpu().numpy().astype(np.float64)
    assert np.abs(dm_only).max() > 0
    assert np.abs(both.cpu().numpy() - (got + dm_only[:, None])).max() <= 4 * ec + 1e-6 * np.abs(got).max()
    # the mask; and however the environments are split into calls, the same bits
    parts = _planes(sim, K)
    nat.trace(sim, off, dm1, parts, env_begin=0, env_count=1)
    nat.trace(sim, off, dm1, parts, env_begin=1, env_count=2)
    assert torch.equal(parts, both)
    masked = _planes(sim, K)
    nat.trace(sim, off, dm1, masked, mask=True)
    assert torch.equal(masked, both * torch.as_tensor(s.mpupil, device=DEV)[None, None])


def test_trace_bits_of_the_single_star(traced):
    """K = 1, theta = 0 is k_lgs_trace bit for bit, atmosphere and mirrors; the on-axis star of constellation B equals
    its K = 1 call bit for bit"""
    s, sysm, sim, scr, nat = traced
    lgs = L.NativeLgs(s, 3, None, device=DEV)
    for gsalt in (90e3, np.inf):
        off, dm1, delta = T.constellation_offsets(sysm, [(0., 0., gsalt)])
        one = _planes(sim, 1)
        nat.trace(sim, off, dm1, one)
        lgs.trace(sim, delta[0])
        assert torch.equal(one[:, 0], sim.t["wfs_phase"]) and one.abs().max() > 0
        nat.trace(sim, off, dm1, one, atm=True, dms=False)
        lgs.trace(sim, delta[0], atm=True, dms=False)
        assert torch.equal(one[:, 0], sim.t["wfs_phase"])
    sim.raytrace_wfs(atm=True, dms=True, reset=True)                   # the natural star: today's trace
    assert torch.equal(_one_plane(nat, sim, sysm, [(0., 0., np.inf)]), sim.t["wfs_phase"])
    offb, dm1b, _ = T.constellation_offsets(sysm, tc.STARS_B)
    plb = _planes(sim, 3)
    nat.trace(sim, offb, dm1b, plb)
    for k in range(3):
        assert torch.equal(plb[:, k], _one_plane(nat, sim, sysm, [tc.STARS_B[k]])), k


def _one_plane(nat, sim, sysm, star):
    off, dm1, _ = T.constellation_offsets(sysm, star)
    pl = _planes(sim, 1)
    nat.trace(sim, off, dm1, pl)
    return pl[:, 0]


def test_trace_refusals(traced):
    s, sysm, sim, scr, nat = traced
    off, dm1, _ = T.constellation_offsets(sysm, tc.STARS_B)
    pl = _planes(sim, 3)
    keep = pl.clone()
    with pytest.raises(Exception, match=r"9 stars: 1\.\.8"):
        nat.trace(sim, np.zeros((9, 3, 2)) + 20, np.zeros((9, 3)), _planes(sim, 9))
    with pytest.raises(Exception, match="offsets for 2 layers, the context has 3"):
        nat.trace(sim, off[:, :2], dm1[:, :2], pl)
    bad = off.copy()
    bad[1, 2, 0] = np.nan
    with pytest.raises(Exception, match="off of star 1, layer 2 is not finite"):
        nat.trace(sim, bad, dm1, pl)
    bad = dm1.copy()
    bad[2, 1] = -1.5
    with pytest.raises(Exception, match="dm1 of star 2, layer 1"):
        nat.trace(sim, off, bad, pl)
    bad = off.copy()
    bad[1, 2, 1] += 200.
    with pytest.raises(Exception, match="footprint of star 1 leaves screen 2"):
        nat.trace(sim, bad, dm1, pl)
    with pytest.raises(Exception, match="environments"):
        nat.trace(sim, off, dm1, pl, env_begin=2, env_count=2)
    with pytest.raises(ValueError, match="planes must be"):
        nat.trace(sim, off, dm1, pl[:, :2])
    assert torch.equal(pl, keep)                        # a refused call wrote nothing


# ------------------------------------------------------------------------------------------------ 2. the covariance
@pytest.mark.parametrize("name", ["A", "B"])
def test_covariance_against_the_statement(name):
    """45 row points and 61 column points (no multiple of the 16 x 16 tile, more than one workgroup per axis):
    rectangular C_0S (science direction against the stars) and square C_SS; constellation B has delta_a != delta_b"""
    stars = tc.STARS_A if name == "A" else tc.STARS_B
    nat = T.NativeTomo(DEV)
    lay = tc.layers_of(tc.LAYERS_3, L0=[25., 1e5, 2.0])              # (L0 = 2 m: both branches of the structure function)
    px, py = tc.points(45, 1)
    qx, qy = tc.points(61, 2)
    for sa, sb, ax, ay, bx, by in ((SCI, stars, px, py, qx, qy), (stars, stars, qx, qy, None, None)):
        want, mag = T.slope_covariance(ax, ay, 0.2, sa, sb, lay, bx, by, return_abs=True)
        got = nat.covariance(ax, ay, 0.2, sa, sb, lay, bx, by)
        again = nat.covariance(ax, ay, 0.2, sa, sb, lay, bx, by)
        assert got.dtype == torch.float64 and tuple(got.shape) == want.shape and torch.equal(got, again)
        err = np.abs(got.cpu().numpy() - want) / mag
        print("constellation %s, %r: largest |device - statement| / sum |w D| = %.3e" % (name, want.shape, err.max()))
        assert err.max() <= 1e-12
    with pytest.raises(Exception, match="not above the highest layer"):
        nat.covariance(px, py, 0.2, [(0., 0., 9000.)], SCI, lay)
    with pytest.raises(Exception, match="d = "):
        nat.covariance(px, py, 0., SCI, SCI, lay)


# ------------------------------------------------------------------------------------------------ the 10x10 system
@pytest.fixture(scope="module")
def loop():
    """(supervisor on one layer at 8000 m, calibrated sensor on constellation A), 4 environments"""
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(tc.params(tc.LAYERS_1), RL, NENV)
    sen = T.LaserTomography(sup, tc.STARS_A)
    ct = sen.calibrate()
    print("calibration: doubled-push deviation %.3e, the stars' responses to one mode differ by %.3e of the response, "
          "cond %.3e" % (sen.linearity, sen.star_match, sen.cond))
    assert ct.shape == (sup.s.nactu, 4 * sen.nslope) and np.isfinite(ct).all()
    return sup, sen


# ------------------------------------------------------------------------------------------------ 3. the sensor
def test_calibration_against_the_host(loop):
    """R from the device's covariances against R from the host's statement: relative error <= cond 1e-12"""
    sup, sen = loop
    assert sen.star_match <= 1e-3 and sen.linearity < 0.05
    c0 = T.slope_covariance(sen.px, sen.py, sen.subapd, SCI, sen.con, sen.layers)
    cs = T.slope_covariance(sen.px, sen.py, sen.subapd, sen.con, sen.con, sen.layers)
    R, cond = T.tomo_reconstructor(c0, cs, sen.noise_var_used, sen.ridge, return_cond=True)
    rel = np.abs(sen.R - R).max() / np.abs(R).max()
    print("R: device against host: relative error %.3e, allowance cond 1e-12 = %.3e (cond %.3e, host's %.3e)" % (
        rel, sen.cond * 1e-12, sen.cond, cond))
    assert rel <= sen.cond * 1e-12
    ns = sen.nslope
    assert np.abs(sen.cmat_tomo - sen.cmat_lgs @ sen.R).max() == 0
    Rsum = sen.R.reshape(ns, 4, ns).sum(axis=1)
    assert np.abs(sen.G - sen.cmat_lgs @ (Rsum - np.eye(ns)) @ sen.D).max() <= 1e-12 * max(np.abs(sen.G).max(), 1e-30)
    assert sen.estimate(np.ones((2, 4 * ns))).shape == (2, ns)


def test_two_stars_in_one_direction():
    """equal noise-free slopes and different noisy ones (each star draws with its own seed); the simulator's frame
    counter advances by one per noisy measure"""
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(tc.params(tc.LAYERS_1), RL, 2)
    sen = T.LaserTomography(sup, [(10., 5., 90e3), (10., 5., 90e3)], noise=0.5)
    sup.reset()
    sup.sim.move_atmos()
    ns = sen.nslope
    sen.trace()
    S = sen.measure(noise=False).clone()
    assert torch.equal(S[:, :ns], S[:, ns:]) and S.abs().max() > 0
    f0 = sup.sim.t["frame"].clone()
    N = sen.measure(noise=True).clone()
    assert not torch.equal(N[:, :ns], N[:, ns:]) and (N - S).abs().max() > 1e-3
    assert torch.equal(sup.sim.t["frame"], f0 + 1)
    want = (sup.sim.t["seeds"].cpu().numpy().view(np.uint32).astype(np.int64)[:, None] + (np.arange(2) + 1) * T.SEED_STRIDE) % (1 << 32)
    assert np.array_equal(sen._seeds.cpu().numpy().view(np.uint32).astype(np.int64), want)


def _bare(sup, nframes):
    sup.reset()
    sup.next_part_one()
    for _ in range(nframes):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()
    return float(sup.get_strehl()[:, 1].mean())


def _bits(sup):
    return [t.clone() for t in (sup.get_slopes(), sup.get_command(), sup.get_err(), sup.get_strehl())]


def test_refusals_and_stop(loop):
    sup, sen = loop
    _bare(sup, 4)
    before = _bits(sup)
    with pytest.raises(ValueError, match=r"0 stars: 1\.\.8"):
        T.LaserTomography(sup, [])
    with pytest.raises(ValueError, match=r"9 stars: 1\.\.8"):
        T.LaserTomography(sup, T.ring(9, 5.))
    with pytest.raises(ValueError, match="gsalt = 8000 m is not above the highest layer"):
        T.LaserTomography(sup, [(0., 0., 8000.)])
    with pytest.raises(ValueError, match="leaves screen 0"):
        T.LaserTomography(sup, [(70., 0., 90e3)])
    with pytest.raises(ValueError, match="reconstructor"):
        T.LaserTomography(sup, tc.STARS_A, reconstructor="glao")
    keep_alt, sup.s.dms[0].alt = sup.s.dms[0].alt, 1000.
    try:
        with pytest.raises(NotImplementedError, match="conjugated to 1000 m"):
            T.LaserTomography(sup, tc.STARS_A)
    finally:
        sup.s.dms[0].alt = keep_alt
    fresh = T.LaserTomography(sup, tc.STARS_A)
    with pytest.raises(RuntimeError, match="calibrate"):
        fresh.start()
    with pytest.raises(RuntimeError, match="calibrate"):
        fresh.set_atmosphere(r0=0.1)
    # the row's refusals: it is the LGS row
    sup.reset_prefetch = "same"
    with pytest.raises(RuntimeError, match="LgsSensor.start: a prefetched reset"):
        sen.start()
    sup.reset_prefetch = None
    sup.sim._twin = object()
    try:
        with pytest.raises(RuntimeError, match="frame pipeline"):
            sen.start()
    finally:
        sup.sim._twin = None
    sup.pyramid = object()
    try:
        with pytest.raises(RuntimeError, match="pyramid is attached"):
            sen.start()
    finally:
        sup.pyramid = None
    sen.start()
    try:
        assert sup.lgs is sen and sup.get_slopes() is sen.est
        other = L.LgsSensor(sup)
        other.cmat = sen.cmat_lgs
        with pytest.raises(RuntimeError, match="LGS attached already"):
            other.start()
        with pytest.raises(RuntimeError, match="stop"):
            sen.calibrate()
        _bare(sup, 4)
        assert tuple(sup.get_slopes().shape) == (NENV, sen.nslope)
        assert np.abs(sen.estimate() - sen.est.double().cpu().numpy()).max() <= 1e-4 * float(sen.est.abs().max())
    finally:
        sen.stop()
    assert sup.lgs is None and sup.sensing is None
    _bare(sup, 4)                                       # stop() gives the loop back bit for bit
    assert all(torch.equal(a, b) for a, b in zip(before, _bits(sup)))


# ------------------------------------------------------------------------------------------------ 4. closed loop
def test_closed_loop(loop):
    """One layer at 8000 m, constellation A (at 20 arcsec the stars' footprints at 8 km are 0.78 m off axis on a 2 m
    pupil), 4 environments, 300 frames from the same seeds: the long-exposure Strehl of the MMSE reconstructor with the
    pseudo-open-loop term above the stars' mean.  Beside them, printed: the NGS integrator, one on-axis LGS, polc=False."""
    sup, sen = loop
    out = {"NGS integrator": _bare(sup, 300)}
    one = L.LgsSensor(sup, gsalt=90e3)
    one.cmat, one.linearity = sen.cmat_lgs, sen.linearity          # the same mirrors, kernels and photometry: star 0's
    one.set_ref(sen.ref)
    one.start()
    try:
        out["one on-axis LGS"] = _bare(sup, 300)
    finally:
        one.stop()
    for rec, polc in (("mean", False), ("tomo", True), ("tomo", False)):
        sen.set_reconstructor(rec, polc)
        sen.start()
        try:
            out["%s%s" % (rec, ", polc" if polc else "")] = _bare(sup, 300)
            assert torch.isfinite(sup.get_command()).all()
        finally:
            sen.stop()
    sen.set_reconstructor("tomo", True)
    print("long-exposure Strehl, 300 frames: " + ", ".join("%s %.4f" % kv for kv in out.items()))
    assert out["tomo, polc"] > out["mean"]


# ------------------------------------------------------------------------------------------------ 5. the environment
def test_environment(loop):
    from ao_marl_amd.env import VecAoEnv
    _, sen = loop
    env = VecAoEnv(tc.params(tc.LAYERS_1), NENV, RL, n_agents_modal=1, frame_pipeline=False)
    esup = env.supervisor
    mine = T.LaserTomography(esup, tc.STARS_A)
    mine.calibrate()
    assert np.abs(mine.R - sen.R).max() <= 1e-9 * np.abs(sen.R).max()
    s_plain = env.reset()
    mine.start()
    try:
        assert not env._native_step_ok(False)
        s = env.reset()
        assert s.shape == s_plain.shape
        zero = torch.zeros(NENV, env.action_dim, device=DEV)
        for _ in range(5):
            s, r, _, _ = env.step(zero, linear_control=True)
        s, r, _, _ = env.step(zero)
        assert s.shape == s_plain.shape and torch.isfinite(s).all() and r.shape[0] == NENV and torch.isfinite(r).all()
        assert tuple(esup.get_slopes().shape) == (NENV, mine.nslope) and esup.get_command().abs().max() > 0
    finally:
        mine.stop()
