"""Modal predictive control on the GPU: the native predictor bank (aomarl_predictor_*) against its float64 statement
(predictive.PredictorBank) through push, set / get / restart / freeze, every attach refusal and attach -> detach against a
context that never had a predictor, the hook in aomarl_do_control and aomarl_rl_control_modes, and the closed loop
against the scalar and the off-line optimised modal integrator."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import libaomarl as la  # noqa: E402
from ao_marl_amd import modal_gains as mg  # noqa: E402
from ao_marl_amd import predictive as pc  # noqa: E402

NAME = "production_sh_10x10_2m"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
NENV, NM, T = 3, 37, 300          # 111 series: one full wave and a ragged one
ZERO = (5, 70)                    # all-zero series: the cap branch runs on the device


def _series():
    """coloured float32 series, a different colour and size per mode; two of them all zero"""
    rng = np.random.default_rng(11)
    S = NENV * NM
    a = np.zeros((T, S))
    pole = np.linspace(0.5, 0.98, S)
    for t in range(1, T):
        a[t] = pole * a[t - 1] + rng.standard_normal(S)
    x = a * np.linspace(0.02, 2.0, S) + 0.1 * rng.standard_normal((T, S))
    x[:, list(ZERO)] = 0.0
    return np.ascontiguousarray(x.reshape(T, NENV, NM), dtype=np.float32)


X32 = _series()


def _ulp_ok(c, cr):
    return (np.abs(c.astype(np.float64) - cr.astype(np.float64)) <= np.spacing(np.abs(cr))).all()


def _close(got, want):
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)


# ------------------------------------------------------------------------------------------------ (1) the bank
@pytest.mark.parametrize("order", (1, 2, 5, 8))
def test_bank_is_the_float64_statement(order):
    """(1) 3 x 37 series, 300 frames, delays 0 / 0.4 / 1 / 1.6, forget 1 / 0.98: theta, P, J, J0 to 1e-9 of each array's
    maximum (the bound of the double filter banks; FMA contraction and one reciprocal per frame are the differences), c to
    one float32 ulp, the zero series' theta bit-equal to its start; one push of 300 == 300 pushes of 1 == 7 + 293 == a
    second run, bit for bit.  p0 = 100, the ridge test's: the series' sizes span 0.02 .. 20, and at p0 = 1e4 (p0 x^2 up to
    1e6) the first updates cancel six digits of P -- there the statement's own float64 differs from its long double by
    1e-10 of a series' maximum in c, six ulp of a c near a zero crossing; at p0 = 100 by 1e-12 (theta: 1.5e-13)."""
    p0 = 100.0
    xd = torch.as_tensor(X32, device="cuda:0")
    start = np.zeros(order)
    start[0] = 1.0
    worst = dict(theta=0.0, P=0.0, J=0.0, J0=0.0)
    for delay in (0.0, 0.4, 1.0, 1.6):
        for forget in (1.0, 0.98):
            def bank():
                return pc.NativePredictorBank(NENV, NM, order, delay, forget, p0, 20)
            b = bank()
            c = b.push(xd).cpu().numpy()
            th, P, J, J0, counts = b.get()
            assert counts == dict(frames=T, since=T, learned=T - order - 2)
            ref = pc.PredictorBank(order, b.delay, forget, p0, 20)
            cr = ref.push(X32)
            for k, got, want in (("theta", th, ref.theta), ("P", P, ref.P), ("J", J, ref.J), ("J0", J0, ref.J0)):
                d = _close(got, want)
                worst[k] = max(worst[k], d)
                assert d <= 1e-9, (k, delay, forget, d)
            assert _ulp_ok(c, cr), (delay, forget)
            assert np.array_equal(P, np.swapaxes(P, -1, -2))
            for s in ZERO:
                assert th.reshape(-1, order)[s].tobytes() == start.tobytes()
                assert (c.reshape(T, -1)[:, s] == 0).all()
            tr = np.trace(P, axis1=-2, axis2=-1)
            assert (tr <= order * p0 * (1 + 1e-12)).all()
            runs = []
            b1 = bank()
            c1 = torch.cat([b1.push(xd[t:t + 1]) for t in range(T)]).cpu().numpy()
            runs.append((b1, c1))
            b2 = bank()
            c2 = torch.cat([b2.push(xd[:7]), b2.push(xd[7:])]).cpu().numpy()
            runs.append((b2, c2))
            b3 = bank()
            runs.append((b3, b3.push(xd).cpu().numpy()))
            for other, co in runs:
                assert co.tobytes() == c.tobytes()
                for a, e in zip(other.get()[:4], (th, P, J, J0)):
                    assert a.tobytes() == e.tobytes(), (delay, forget)
                assert other.counts == counts
    print("order %d: worst deviation from the statement, of each array's maximum: %s" % (order, worst))


# ------------------------------------------------------------------------------------------------ (2) set / get
def test_set_get_restart_and_freeze():
    """(2) set -> get is bit-exact (the upper triangle is what is kept); restart: no update for n + 2 frames, J carries
    over and is not counted for nskip frames; set_learning(0): theta and P bit-equal while c, J, J0 go on; every refusal
    of create and set names its field."""
    n = 4
    xd = torch.as_tensor(X32, device="cuda:0")
    rng = np.random.default_rng(3)
    b = pc.NativePredictorBank(NENV, NM, n, 1.6, 0.99, 1e4, 20)
    th0 = rng.standard_normal((NENV, NM, n))
    A = rng.standard_normal((NENV, NM, n, n))
    P0 = A @ np.swapaxes(A, -1, -2) + np.eye(n)
    P0 = np.triu(P0) + np.swapaxes(np.triu(P0, 1), -1, -2)
    b.set(th0, P0)
    th, P, J, J0, counts = b.get()
    assert th.tobytes() == th0.tobytes() and P.tobytes() == P0.tobytes() and (J == 0).all() and (J0 == 0).all()
    assert counts == dict(frames=0, since=0, learned=0)
    b.set(theta=th0 * 2)
    assert b.theta.tobytes() == (th0 * 2).tobytes() and b.P.tobytes() == P0.tobytes()
    # the statement from the same state
    ref = pc.PredictorBank(n, b.delay, 0.99, 1e4, 20)
    ref.set(th0 * 2, P0)
    c = b.push(xd[:100]).cpu().numpy()
    cr = ref.push(X32[:100])
    assert _ulp_ok(c, cr) and _close(b.theta, ref.theta) <= 1e-9 and _close(b.P, ref.P) <= 1e-9
    # restart
    th, P, J, J0, _ = b.get()
    b.restart()
    assert b.counts == dict(frames=100, since=0, learned=100 - n - 2)
    b.push(xd[100:100 + n + 2], want_c=False)
    a = b.get()
    assert a[0].tobytes() == th.tobytes() and a[1].tobytes() == P.tobytes() and a[2].tobytes() == J.tobytes()
    b.push(xd[100 + n + 2:100 + n + 3], want_c=False)
    a = b.get()
    live = np.ones(NENV * NM, bool)
    live[list(ZERO)] = False
    assert (a[0].reshape(-1, n)[live] != th.reshape(-1, n)[live]).any(axis=1).all() and a[2].tobytes() == J.tobytes()
    b.push(xd[100 + n + 3:121], want_c=False)
    a = b.get()
    assert (a[2].reshape(-1)[live] != J.reshape(-1)[live]).all()
    assert a[4] == dict(frames=121, since=21, learned=100 - n - 2 + 21 - n - 2)
    ref.restart()
    ref.push(X32[100:121])
    assert _close(a[0], ref.theta) <= 1e-9 and _close(a[2], ref.J) <= 1e-9
    # frozen
    th, P, J, J0, _ = a
    b.learning = False
    ref.learning = False
    c = b.push(xd[121:200]).cpu().numpy()
    cr = ref.push(X32[121:200])
    a = b.get()
    assert a[0].tobytes() == th.tobytes() and a[1].tobytes() == P.tobytes()
    assert (a[2].reshape(-1)[live] != J.reshape(-1)[live]).all() and (a[3].reshape(-1)[live] != J0.reshape(-1)[live]).all()
    assert a[4]["learned"] == 100 - n - 2 + 21 - n - 2 and _ulp_ok(c, cr) and _close(a[2], ref.J) <= 1e-9
    x_last, c_last = b.last()
    assert torch.equal(x_last, xd[199]) and np.array_equal(c_last.cpu().numpy(), c[-1])
    b.learning = True
    b.push(xd[200:201], want_c=False)
    assert (b.theta != th).any()
    # refusals
    thk, Pk = b.theta, b.P
    for kw, word in ((dict(order=0), "order"), (dict(order=9), "order"), (dict(forget=0.0), "forget"), (dict(forget=1.5), "forget"),
                     (dict(p0=0.0), "p0"), (dict(p0=float("nan")), "p0"), (dict(delay=2.5), "delay"), (dict(nskip=-1), "nskip"),
                     (dict(nenv=0), "nenv")):
        a = dict(nenv=2, nmodes=4, order=2, delay=1.0, forget=1.0, p0=1e4, nskip=0)
        a.update(kw)
        with pytest.raises(la.AomarlError, match=word):
            pc.NativePredictorBank(**a)
    bad = P0.copy()
    bad[1, 2, 0, 1] += 1e-3
    with pytest.raises(la.AomarlError, match="not symmetric"):
        b.set(P=bad)
    bad = P0.copy()
    bad[0, 0, 2, 2] = -1.0
    with pytest.raises(la.AomarlError, match="not positive"):
        b.set(P=bad)
    bad = th0.copy()
    bad[2, 5, 1] = np.inf
    with pytest.raises(la.AomarlError, match="theta"):
        b.set(theta=bad)
    assert b.P.tobytes() == Pk.tobytes() and b.theta.tobytes() == thk.tobytes()         # (a refused set changes nothing)
    with pytest.raises(ValueError):
        b.push(torch.zeros(2, NENV, NM + 1, device="cuda:0"))


# ------------------------------------------------------------------------------------------------ environments
def _env(nenv, delay=None, **kw):
    from ao_marl_amd import params
    from ao_marl_amd.env import VecAoEnv
    ps = params.builtin(NAME)
    if delay is not None:
        ps.p_controllers[0].delay = float(delay)
    kw.setdefault("frame_pipeline", False)
    return VecAoEnv(ps, nenv, RL, n_agents_modal=1, **kw)


def _mgain(nm):
    return np.linspace(0.3, 1.2, nm).astype(np.float32)


GAIN = 0.4


# ------------------------------------------------------------------------------------------------ (3) attach
def test_attach_refusals():
    """(3) attach without modal gains, with an on-line optimiser attached (and the optimiser with a predictor attached),
    with per-environment scalar gains, with other sizes, a second attach, destroy and push while attached,
    set_modal_gains(None) while attached, do_control on a partial range: each refused by name; a do_control with gain 0
    feeds nothing; the context works on afterwards."""
    env = _env(3)
    sup, sim = env.supervisor, env.supervisor.sim
    nm = sup.nmodes
    sup.set_gain(GAIN)
    sup.ensure_slopes2modes()
    lib = sim.lib

    def bank(nenv=3, nmodes=nm):
        return pc.NativePredictorBank(nenv, nmodes, 2, 1.0)
    with pytest.raises(la.AomarlError, match="no modal gains"):
        bank().attach(sim)
    sup.set_modal_gains(_mgain(nm))
    with pytest.raises(la.AomarlError, match="nmodes"):
        bank(nmodes=nm + 1).attach(sim)
    with pytest.raises(la.AomarlError, match="nenv = 2"):
        bank(nenv=2).attach(sim)
    sup.set_gain(np.full(3, 0.3, dtype=np.float32))
    with pytest.raises(la.AomarlError, match="per-environment scalar gains"):
        bank().attach(sim)
    sup.set_gain(GAIN)
    on = mg.NativeOnlineLoopBank(3, nm, [0.1, 0.3], 1.0, pool="all", chunk=4)
    on.attach(sim)
    with pytest.raises(la.AomarlError, match="on-line modal-gain optimiser is attached"):
        bank().attach(sim)
    on.detach()
    b = bank()
    b.attach(sim)
    with pytest.raises(la.AomarlError, match="modal predictor is attached"):
        on.attach(sim)
    with pytest.raises(la.AomarlError, match="attached already"):
        bank().attach(sim)
    assert lib.aomarl_predictor_destroy(b.ptr) != 0 and b"attached" in lib.aomarl_last_error()
    with pytest.raises(la.AomarlError, match="aomarl_do_control feeds it"):
        b.push(torch.zeros(1, 3, nm, device="cuda:0"))
    with pytest.raises(la.AomarlError, match="modal predictor is attached"):
        sup.set_modal_gains(None)
    sup.set_modal_gains(_mgain(nm))                     # (other values are fine: they are not used)
    sup.reset()
    sup.next_part_two(None, linear_control=True)
    sup.next_part_one(do_control=False)
    with pytest.raises(la.AomarlError, match="partial environment range"):
        sim.do_control(1, 2)
    sim.do_control()
    assert b.counts["frames"] == 1
    sim.set_gain(0.0)                                   # err alone: not a frame of the loop
    sim.do_control()
    sim.set_gain(GAIN)
    assert b.counts["frames"] == 1
    b.detach()
    sim.do_control(1, 2)
    assert b.counts["frames"] == 1
    # the supervisor's front end: one of the two at a time
    pred = pc.ModalPredictor(sup, order=2).start()
    with pytest.raises(RuntimeError, match="modal predictor is attached"):
        mg.OnlineModalGains(sup).start()
    with pytest.raises(RuntimeError, match="already"):
        pc.ModalPredictor(sup).start()
    pred.stop()
    opt = mg.OnlineModalGains(sup, pool="all").start()
    with pytest.raises(RuntimeError, match="on-line modal-gain optimiser"):
        pc.ModalPredictor(sup).start()
    opt.stop()
    # a pipelined frame in flight
    env = _env(3, frame_pipeline=True)
    sup, sim = env.supervisor, env.supervisor.sim
    env.reset()
    zero = torch.zeros(3, env.action_dim, device="cuda:0")
    for _ in range(3):
        env.step(zero)
    if sim.frame_pipeline_state()[0]:
        with pytest.raises(la.AomarlError, match="pipelined frame is in flight"):
            bank().attach(sim)
        s, _, _, _ = env.step(zero)
        assert torch.isfinite(s).all()


def test_detached_is_a_context_that_never_had_one():
    """(3) two environments under the same modal gains, one with a predictor attached and detached before the first step:
    states, rewards, commands and Strehl bit-equal over 5 steps, and the launch counters of a step too."""
    a, b = _env(3), _env(3)
    nm = a.supervisor.nmodes
    for e in (a, b):
        e.supervisor.set_gain(GAIN)
        e.supervisor.set_modal_gains(_mgain(nm))
    pred = pc.ModalPredictor(b.supervisor, order=3).start()
    assert b.supervisor.modal_predictor is pred
    pred.stop()
    assert b.supervisor.modal_predictor is None
    assert np.array_equal(b.supervisor.modal_gains, a.supervisor.modal_gains)
    sa, sb = a.reset(), b.reset()
    assert torch.equal(sa, sb)
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    for it in range(5):
        act = torch.rand(3, a.action_dim, device="cuda:0", generator=gen) * 2 - 1
        if it == 4:
            la.arith_launches(reset=True)
        sa, ra, _, _ = a.step(act)
        if it == 4:
            na = la.arith_launches()
            la.arith_launches(reset=True)
        sb, rb, _, _ = b.step(act)
        if it == 4:
            nb = la.arith_launches()
        assert torch.equal(sa, sb) and torch.equal(ra, rb), it
        assert torch.equal(a.supervisor.sim.strehl, b.supervisor.sim.strehl), it
        assert torch.equal(a.supervisor.sim.com, b.supervisor.sim.com), it
    assert na == nb


# ------------------------------------------------------------------------------------------------ (4) the hook
@pytest.mark.parametrize("mode", ["parts", "env_step_zero", "env_step_random"])
def test_hook_runs_the_predictor_and_commands_with_it(mode):
    """(4) 10x10, 2 environments, 40 frames through next_part_two / next_part_one, and through env.step with zero and with
    random actions: (i) the row the device consumed is slopes2modes() + volts2modes(voltage) of the frame to 1e-6 max|x|;
    (ii) those rows pushed into the statement give the device's c to one ulp; (iii) the command is m2v . c behind the frame
    and m2v . (c + action * freedom on the action modes) in the delay line behind the step, to 5e-4 of max|com|."""
    nfr, n = 40, 3
    env = _env(2)
    sup, sim = env.supervisor, env.supervisor.sim
    nm = sup.nmodes
    pred = pc.ModalPredictor(sup, order=n, nskip=5).start()
    assert np.array_equal(sup.modal_gains, np.ones((1, nm), dtype=np.float32))
    ref = pc.PredictorBank(n, pred.delay, 1.0, 1e4, 5)
    m2v = np.asarray(sup.modes2volts, dtype=np.float64)
    am = np.asarray(sup.action_range) % nm
    fr = np.asarray(sup.freedom_vector, dtype=np.float64)
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    by_step = mode != "parts"
    if by_step:
        env.reset()                                   # frame 0: linear_step
    else:
        sup.reset()
    na = sim.s.nactu
    dmax = cmax = 0.0
    c_prev = None
    for t in range(nfr):
        if by_step:
            if t:
                act = torch.zeros(2, env.action_dim, device="cuda:0") if mode == "env_step_zero" else \
                    torch.rand(2, env.action_dim, device="cuda:0", generator=gen) * 2 - 1
                env.step(act)
                assert env._glue is not None
                # the command the step's head composed went into the delay line: com1 behind apply_control
                modes = c_prev.astype(np.float64).copy()
                modes[:, am] += act.double().cpu().numpy() * fr[am]
                com1 = sim.t["com1"][:, :na].double().cpu().numpy()
                d = np.abs(com1 - modes @ m2v.T).max()
                dmax, cmax = max(dmax, d), max(cmax, np.abs(com1).max())
                assert d <= 5e-4 * np.abs(com1).max(), (t, d)
        else:
            sup.next_part_two(None, linear_control=True)
            sup.next_part_one()
        x, c = pred.bank.last()
        xp = (sim.slopes2modes().double() + sim.volts2modes(sim.voltage).double()).cpu().numpy()
        x = x.cpu().numpy()
        assert np.abs(x - xp).max() <= 1e-6 * np.abs(x).max(), t
        cr = ref.push(x[None])[0]
        c = c.cpu().numpy()
        assert _ulp_ok(c, cr), t
        com = sim.com.double().cpu().numpy()
        d = np.abs(com - c.astype(np.float64) @ m2v.T).max()
        dmax, cmax = max(dmax, d), max(cmax, np.abs(com).max())
        assert d <= 5e-4 * np.abs(com).max(), (t, d)
        c_prev = c
    counts = pred.bank.counts
    assert counts == dict(frames=nfr, since=nfr, learned=nfr - n - 2) == ref.counts
    assert _close(pred.theta, ref.theta) <= 1e-9 and (pred.theta != np.eye(n)[0]).any()
    print("%s: max |com - m2v . modes| %.3g of max|com| %.3g" % (mode, dmax, cmax))
    # a do_control with gain 0 feeds nothing
    sim.set_gain(0.0)
    sim.do_control()
    sim.set_gain(sup.gain)
    assert pred.bank.counts == counts
    # reset() restarts the history: theta carries over, the frame counter starts again
    th = pred.theta
    if by_step:
        env.reset()
    else:
        sup.reset()
    k = pred.bank.counts
    assert k["since"] == (1 if by_step else 0) and pred.theta.tobytes() == th.tobytes()
    pred.stop()
    assert sup.modal_gains is None and sup.modal_predictor is None
    assert pred.theta.tobytes() == th.tobytes()


def test_statement_path_commands_the_same():
    """native=False: the NumPy statement fed through observe() after every next_part_one commands what the device bank
    commands -- 25 frames of two supervisors on the same seeds, com and theta to 5e-4 of their maximum; and it says so
    when an action has been composed on the integrator's modes."""
    a, b = _env(2), _env(2)
    pa = pc.ModalPredictor(a.supervisor, order=3, nskip=5).start()
    pb = pc.ModalPredictor(b.supervisor, order=3, nskip=5, native=False).start()
    with pytest.raises(RuntimeError, match="run by do_control"):
        pa.observe()
    a.supervisor.reset()
    b.supervisor.reset()
    for t in range(25):
        for sup in (a.supervisor, b.supervisor):
            sup.next_part_two(None, linear_control=True)
            sup.next_part_one()
        pb.observe()
        ca, cb = a.supervisor.sim.com, b.supervisor.sim.com
        assert (ca - cb).abs().max().item() <= 5e-4 * ca.abs().max().item(), t
    # (two loops closed through float32 commands: their x differ by float32 round-off from the first frame on, so theta
    # is held to the commands' tolerance, not to the double filter banks')
    assert _close(pb.theta, pa.theta) <= 5e-4 and pb.bank.counts == pa.bank.counts
    r = pb.rejection
    nm = a.supervisor.nmodes                      # (modes the command matrix filters are never excited: 0 / 0)
    assert r.shape == (2, nm) and np.isfinite(r).sum() >= 2 * (nm - RL["n_reverse_filtered_from_cmat"])
    assert (r[np.isfinite(r)] > 0).all() and np.median(r[np.isfinite(r)]) < 1.0
    b.supervisor.last_modes = object()
    with pytest.raises(RuntimeError, match="linear_control=True only"):
        pb.observe()
    b.supervisor.last_modes = None
    pa.stop()
    pb.stop()


def test_save_and_load(tmp_path):
    env = _env(2)
    sup = env.supervisor
    pred = pc.ModalPredictor(sup, order=3, nskip=5).start()
    sup.reset()
    for _ in range(12):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()
    th, P = pred.theta, pred.P
    path = str(tmp_path / "pred.npz")
    pred.save(path)
    pred.stop()
    again = pc.ModalPredictor(sup, order=3, nskip=5).start()
    assert (again.theta != th).any()
    again.load(path)
    assert again.theta.tobytes() == th.tobytes() and again.P.tobytes() == P.tobytes()
    again.stop()
    other = pc.ModalPredictor(sup, order=2).start()
    with pytest.raises(ValueError, match="order"):
        other.load(path)
    other.stop()


# ------------------------------------------------------------------------------------------------ (5) it helps
def _closed_loop_e2(sup, nframes, first=100):
    """mean over frames >= first, environments and modes of the squared residual modes of `nframes` closed-loop frames
    from a fresh reset"""
    sup.reset()
    acc = torch.zeros(sup.sim.nenv, sup.nmodes, dtype=torch.float64, device="cuda:0")
    for t in range(nframes):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()
        if t >= first:
            acc += sup.sim.slopes2modes().double() ** 2
    return float(acc.mean() / (nframes - first))


def _frozen_predictor_e2(sup, order, nframes):
    """the predictor of this order warm-started on one open-loop episode, frozen, then a fresh closed-loop episode"""
    pred = pc.ModalPredictor(sup, order=order).start()
    pred.warm_start(nframes).freeze()
    e2, rms = _closed_loop_e2(sup, nframes), pred.pol_rms
    pred.stop()
    return e2, rms


def test_closed_loop_beats_the_integrators():
    """(5) 10x10, 4 environments, the file's own delay, order 4: a warm start on one open-loop episode, then a fresh
    episode with the filter frozen.  The mean over frames >= 100 and modes of e^2 is below that of the scalar integrator
    and of the off-line optimised modal integrator on the same seeds and frames."""
    nframes = 600
    env = _env(4)
    sup = env.supervisor
    sup.ensure_slopes2modes()
    scalar = _closed_loop_e2(sup, nframes)
    mg.optimize_modal_gains(sup, nrec=nframes, nskip=50)
    modal = _closed_loop_e2(sup, nframes)
    sup.set_modal_gains(None)
    got, rms = _frozen_predictor_e2(sup, 4, nframes)
    print("closed loop, delay %g, mean e^2: scalar integrator (gain %.2f) %.5g, off-line modal gains %.5g, frozen "
          "predictor of order 4 %.5g (%.3f of the scalar, %.3f of the modal integrator); POL rms %.4g"
          % (sup.s.delay, sup.gain, scalar, modal, got, got / scalar, got / modal, rms))
    assert np.isfinite(got) and got < scalar
    assert got < modal
