"""Per-mode integrator gains on the GPU: the native loop-filter bank (aomarl_modopti_*) against its float64 statement
(ao_marl_amd/modal_gains.py), the law m[t] = m[t-1] + gain * mgain[m] * e[t] on every control path of the 10x10 system,
ones against no gains, the guards, and the optimiser against its own prediction in closed loop."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import libaomarl as la  # noqa: E402
from ao_marl_amd import modal_gains as mg  # noqa: E402

NAME = "production_sh_10x10_2m"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
CHUNK = 64
DELAYS = (0.0, 0.5, 1.0, 1.5, 2.0)


# ------------------------------------------------------------------------------------------------ (d) the bank
def _grid(ngain):
    # 1: one stable gain; 7: up to 1.2; 33: up to 2.2 -- unstable candidates at every delay
    return {1: np.array([0.3]), 7: np.linspace(0.0, 1.2, 7), 33: np.linspace(0.0, 2.2, 33)}[ngain]


@pytest.mark.parametrize("delay", DELAYS)
def test_bank_is_the_float64_statement(delay):
    """(d) J at rtol 1e-9 for candidates whose pole radius is at most 0.99: at most 3 chunk + 5 = 197 frames x 1.1e-16 x
    the amplification 1 / (1 - 0.99) = 100 is 2e-12, FMA contraction being the only difference; one call and two calls
    give equal bits; the argmin is the statement's wherever its best and second-best J differ by more than 1e-8
    relative (pairs left out for that: at most 1 %); exact ties -- one counted frame, none, an all-zero series -- go by
    the tie rule on both sides; an unstable candidate is never chosen."""
    nenv, total, left_out = 3, 0, 0
    rng = np.random.default_rng(100 + int(10 * delay))
    for nmodes in (5, 64, 87):
        for frames in (1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5):
            # a random walk plus white noise, a different mix per mode; one all-zero (filtered) series
            x = np.cumsum(rng.standard_normal((frames, nenv, nmodes)), axis=0) * np.linspace(0.1, 1.5, nmodes) + \
                rng.standard_normal((frames, nenv, nmodes))
            x[:, 0, nmodes // 2] = 0.0
            x32 = np.ascontiguousarray(x, dtype=np.float32)
            xd = torch.as_tensor(x32, device="cuda:0")
            for ngain in (1, 7, 33):
                for nskip in (0, 10):
                    one = mg.NativeLoopBank(nenv, nmodes, _grid(ngain), delay, nskip).accumulate(xd)
                    J, arg, st, n = one.result()
                    h = frames // 2
                    two = mg.NativeLoopBank(nenv, nmodes, _grid(ngain), delay, nskip).accumulate(xd[:h]).accumulate(xd[h:])
                    J2, arg2, _, n2 = two.result()
                    assert n == n2 == frames
                    assert np.array_equal(J, J2) and np.array_equal(arg, arg2), (nmodes, frames, ngain, nskip)
                    gains = one.gains
                    ref = mg.LoopBank(gains, delay, nskip).accumulate(x32)
                    Jr, argr, str_ = ref.result()
                    assert (st == str_).all()
                    ok = mg.pole_radius(gains, delay) <= 0.99
                    ok |= gains == 0.0                     # the open loop: e = x
                    np.testing.assert_allclose(J[..., ok], Jr[..., ok], rtol=1e-9, atol=0)
                    assert (arg >= 0).all() and st[arg].all()
                    # best against second best of the statement, among the stable candidates
                    Js = np.sort(np.where(st, Jr, np.inf), axis=-1)
                    if st.sum() > 1:
                        gap = (Js[..., 1] - Js[..., 0]) / np.maximum(Js[..., 1], 1e-300)
                        tie = Js[..., 1] == Js[..., 0]
                    else:
                        gap, tie = np.ones(Js.shape[:-1]), np.zeros(Js.shape[:-1], bool)
                    clear = tie | (gap > 1e-8)
                    assert (arg[clear] == argr[clear]).all(), (nmodes, frames, ngain, nskip)
                    assert arg[0, nmodes // 2] == int(np.argmin(np.where(st, gains, np.inf)))      # the zero series
                    total += clear.size
                    left_out += int((~clear).sum())
    assert left_out <= 0.01 * total, (left_out, total)


def test_bank_refusals_name_the_argument():
    for kw, word in ((dict(delay=2.5), "delay"), (dict(delay=-0.5), "delay"), (dict(gains=[]), "ngain"),
                     (dict(gains=[0.1, float("nan")]), r"gains\[1\]"), (dict(nskip=-1), "nskip"), (dict(nenv=0), "nenv")):
        a = dict(nenv=2, nmodes=4, gains=[0.1, 0.2], delay=1.0, nskip=0)
        a.update(kw)
        with pytest.raises(la.AomarlError, match=word):
            mg.NativeLoopBank(**a)
    b = mg.NativeLoopBank(2, 4, [0.1, 0.2], 1.0)
    with pytest.raises(ValueError):
        b.accumulate(torch.zeros(3, 2, 5, device="cuda:0"))
    lib = la.load()
    x = torch.zeros(2, 8, device="cuda:0")
    assert lib.aomarl_modopti_accumulate(b.ptr, x.data_ptr(), 1, 7, None) != 0 and b"frame_stride" in lib.aomarl_last_error()


# ------------------------------------------------------------------------------------------------ environments
def _env(nenv, delay=None, **kw):
    from ao_marl_amd import params
    from ao_marl_amd.env import VecAoEnv
    ps = params.builtin(NAME)
    if delay is not None:
        ps.p_controllers[0].delay = float(delay)
    kw.setdefault("frame_pipeline", False)
    return VecAoEnv(ps, nenv, RL, n_agents_modal=1, **kw)


def _mgain(nm, nenv=None):
    base = np.linspace(0.3, 1.2, nm).astype(np.float32)
    if nenv is None:
        return base
    return (base[None, :] * (1.0 - 0.07 * np.arange(nenv, dtype=np.float32))[:, None]).astype(np.float32)


def _rollout(env, T, by_env_step):
    """T closed-loop frames from reset with zero actions: e[t] (residual modes) and m[t] = v2m . com[t] of every frame"""
    sup, sim = env.supervisor, env.supervisor.sim
    E, M = [], []
    if by_env_step:
        env.reset()                                   # frame 0: linear_step
        zero = torch.zeros(env.nenv, env.action_dim, device="cuda:0")
        for t in range(T):
            if t:
                env.step(zero)
                assert env._glue is not None          # the one-call step took it
            E.append(env._res_modes.double().cpu().numpy())
            M.append(sim.volts2modes(sup.get_command()).double().cpu().numpy())
    else:
        sup.reset()
        for t in range(T):
            sup.next_part_two(None, linear_control=True)
            sup.next_part_one()                       # aomarl_next_part_one: do_control inside
            E.append(sim.slopes2modes().double().cpu().numpy())
            M.append(sim.volts2modes(sim.com).double().cpu().numpy())
    return np.stack(E), np.stack(M)


GAIN = 0.4        # gain * mgain in [0.12, 0.48]: stable at delay 1 (< 1) and at delay 2 (< 0.618)


@pytest.mark.parametrize("delay", [None, 2.0])
@pytest.mark.parametrize("by_env_step", [False, True])
@pytest.mark.parametrize("per_env", [False, True])
def test_law_and_bank_are_the_same_recursion(delay, by_env_step, per_env):
    """(e) 64 closed-loop frames of 3 environments under a non-uniform mgain, call by call and through env_step:
    (i)  m[t] - m[t-1] = gain * mgain (.) e[t] to 2e-5 x max|m| (the round trip through m2v and v2m, the tolerance of
         test_modal_shortcut_equals_full_projection_path);
    (ii) with x[t] = e[t] + wa m[t-1] + wb m[t-2] + wc m[t-3] built from the readings, the bank run on a grid that holds
         every gain * mgain[m] returns J = sum e[t]^2 at that gain.  Tolerance: (i) lets m leave the exact recursion by
         d = 2e-5 max|m| per frame, T d after T frames, times at most 3 for the loop's peaking at these gains: the
         bank's e differs by D <= 3 T d per frame, so |J_bank - J| <= 2 D sqrt(T J) + T D^2 (Cauchy-Schwarz)."""
    T = 64
    env = _env(3, delay)
    sup, sim = env.supervisor, env.supervisor.sim
    nm = sup.nmodes
    mgain = _mgain(nm, 3 if per_env else None)
    sup.set_gain(GAIN)
    sup.set_modal_gains(mgain)
    got = sup.modal_gains
    assert got.shape == ((3, nm) if per_env else (1, nm)) and np.array_equal(got.reshape(mgain.shape), mgain)
    E, M = _rollout(env, T, by_env_step)
    g = (np.float32(GAIN) * np.broadcast_to(mgain, (3, nm))).astype(np.float32)      # the device's fp32 product
    scale = np.abs(M).max()
    assert scale > 0 and np.abs(E).max() > 0
    Mprev = np.concatenate([np.zeros_like(M[:1]), M[:-1]])
    dev = np.abs(M - Mprev - g.astype(np.float64) * E).max()
    print("law: max deviation %.3g of max|m| %.3g" % (dev, scale))
    assert dev <= 2e-5 * scale
    # the scalar law would be off by (1 - mgain) gain e
    assert np.abs(M - Mprev - GAIN * E).max() > 100 * 2e-5 * scale
    wa, wb, wc = mg.delay_weights(sup.s.delay)
    Z = np.zeros_like(M[:1])
    x = E + wa * np.concatenate([Z, M[:-1]]) + wb * np.concatenate([Z, Z, M[:-2]]) + wc * np.concatenate([Z, Z, Z, M[:-3]])
    grid = np.unique(g)
    bank = mg.NativeLoopBank(3, nm, grid, sup.s.delay, 0).accumulate(torch.as_tensor(x.astype(np.float32), device="cuda:0"))
    J, _, st, n = bank.result()
    assert n == T and st.all()
    idx = np.searchsorted(grid, g)
    assert (grid[idx] == g).all()
    Jb = np.take_along_axis(J, idx[..., None], axis=-1)[..., 0]
    Jw = (E ** 2).sum(axis=0)
    D = 3 * T * 2e-5 * scale
    print("bank: max |J_bank - J| / tolerance %.3g" % (np.abs(Jb - Jw) / (2 * D * np.sqrt(T * Jw) + T * D * D)).max())
    assert (np.abs(Jb - Jw) <= 2 * D * np.sqrt(T * Jw) + T * D * D).all()
    # and the native bank is the statement on one grid per series
    Jp = mg.loop_rejection(x.astype(np.float32), g.astype(np.float64)[..., None], sup.s.delay)[..., 0]
    np.testing.assert_allclose(Jb, Jp, rtol=1e-9)


def test_ones_change_nothing():
    """(f) mgain = ones against no modal gains: aomarl_rl_control_modes bit for bit; a 12-step env_step rollout bit for
    bit against the chain modal gains run (the general chain: states, rewards, Strehl; the small systems' two-kernel
    chain is by its own statement only round-off-equal to it, and is compared at the modal tolerance); aomarl_do_control
    to 2e-5 x max|m|; with the gains cleared the launch counters of an env_step are a fresh environment's."""
    a, b, c = _env(3), _env(3), _env(3)
    nm = a.supervisor.nmodes
    b.fused_tail = False                                 # no gains, general chain
    c.supervisor.set_modal_gains(np.ones(nm, dtype=np.float32))
    sa, sb, sc = a.reset(), b.reset(), c.reset()
    assert torch.equal(sb, sc)
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    for it in range(12):
        act = torch.rand(3, a.action_dim, device="cuda:0", generator=gen) * 2 - 1
        sa, ra, _, _ = a.step(act)
        sb, rb, _, _ = b.step(act)
        sc, rc, _, _ = c.step(act)
        assert torch.equal(sb, sc) and torch.equal(rb, rc), it
        assert torch.equal(b.supervisor.sim.strehl, c.supervisor.sim.strehl), it
        assert torch.equal(b._res_modes, c._res_modes) and torch.equal(b._ring, c._ring), it
        ma, mc = a._ring[a._ring_pos], c._ring[c._ring_pos]
        assert (ma - mc).abs().max().item() <= 2e-5 * ma.abs().max().item(), it
        # do_control ran in Btt coordinates in c, in actuator space in b
        mb = b.supervisor.sim.volts2modes(b.supervisor.get_command())
        mc = c.supervisor.sim.volts2modes(c.supervisor.get_command())
        assert (mb - mc).abs().max().item() <= 2e-5 * mb.abs().max().item(), it
    # aomarl_rl_control_modes on the same operands
    sim = c.supervisor.sim
    m0, m1 = torch.randn(3, nm, device="cuda:0", generator=gen), torch.randn(3, nm, device="cuda:0", generator=gen)
    act = torch.rand(3, sim.nact, device="cuda:0", generator=gen) * 2 - 1
    out1 = sim.rl_control_modes(m0, m1, 0.37, act).clone()
    com1 = sim.com.clone()
    c.supervisor.set_modal_gains(None)
    assert c.supervisor.modal_gains is None
    out0 = sim.rl_control_modes(m0, m1, 0.37, act).clone()
    assert torch.equal(out0, out1) and torch.equal(sim.com, com1)
    # cleared: the fast chains are back
    fresh = _env(3)

    def one_step_counters(env, prepare=None):
        env.reset()
        zero = torch.zeros(3, env.action_dim, device="cuda:0")
        env.step(zero)
        env.step(zero)
        if prepare:
            prepare()
        la.arith_launches(reset=True)
        env.step(zero)
        return la.arith_launches()
    want = one_step_counters(fresh)
    c.supervisor.set_modal_gains(np.ones(nm, dtype=np.float32))
    got = one_step_counters(c, lambda: c.supervisor.set_modal_gains(None))
    assert got == want
    c.supervisor.set_modal_gains(np.ones(nm, dtype=np.float32))
    assert one_step_counters(c) != want                 # (the counters do see the general chain)


def test_guards():
    """(g) a wrong nmodes or nrows is refused with the argument named; negative or non-finite entries too; gains set on a
    frame_pipeline=True environment: the step runs the general chain (never the scalar law); gains set while a
    pipelined frame is in flight are refused, naming aomarl_set_modal_gains."""
    env = _env(3, frame_pipeline=True)
    sup, sim = env.supervisor, env.supervisor.sim
    nm = sup.nmodes
    with pytest.raises(la.AomarlError, match="nmodes"):
        sup.set_modal_gains(np.ones(nm + 1, dtype=np.float32))
    with pytest.raises(ValueError, match="nrows"):
        sup.set_modal_gains(np.ones((2, nm), dtype=np.float32))
    lib = sim.lib
    ones = np.ones((4, nm), dtype=np.float32)
    assert lib.aomarl_set_modal_gains(sim.ctx, la.fptr(ones), 0, nm) != 0 and b"nrows" in lib.aomarl_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        v = np.ones(nm, dtype=np.float32)
        v[7] = bad
        with pytest.raises(la.AomarlError, match=r"mgain\[0\]\[7\]"):
            sup.set_modal_gains(v)
    assert sup.modal_gains is None
    # four rows on a state of three environments: refused where the state is at hand
    assert lib.aomarl_set_modal_gains(sim.ctx, la.fptr(ones), 4, nm) == 0
    sup.ensure_slopes2modes()
    sup.reset()
    with pytest.raises(la.AomarlError, match="nrows = 4"):
        sim.do_control()
    sup.set_modal_gains(None)
    # pipelined environment, gains set before the episode: the general chain
    mgain = _mgain(nm)
    sup.set_gain(GAIN)
    sup.set_modal_gains(mgain)
    E, M = _rollout(env, 16, True)
    assert not sim.frame_pipeline_state()[0]
    g = np.float32(GAIN) * mgain
    Mprev = np.concatenate([np.zeros_like(M[:1]), M[:-1]])
    assert np.abs(M - Mprev - g.astype(np.float64) * E).max() <= 2e-5 * np.abs(M).max()
    assert np.abs(M - Mprev - GAIN * E).max() > 100 * 2e-5 * np.abs(M).max()
    # ... and while a frame is in flight
    sup.set_modal_gains(None)
    env.reset()
    zero = torch.zeros(3, env.action_dim, device="cuda:0")
    for _ in range(3):
        env.step(zero)
    if sim.frame_pipeline_state()[0]:
        with pytest.raises(la.AomarlError, match="aomarl_set_modal_gains"):
            sup.set_modal_gains(mgain)
        assert sup.modal_gains is None
        s, _, _, _ = env.step(zero)
        assert torch.isfinite(s).all()


def test_record_open_loop_refusals():
    from types import SimpleNamespace as NS
    ok = dict(sim=NS(_twin=None), reset_prefetch=None, pure_delay_0=False, autoencoder=None)
    for kw, exc, word in ((dict(reset_prefetch="same"), RuntimeError, "reset_prefetch"),
                          (dict(sim=NS(_twin=object())), RuntimeError, "frame pipeline"),
                          (dict(pure_delay_0=True), NotImplementedError, "modification_online")):
        with pytest.raises(exc, match=word):
            mg.record_open_loop(NS(**dict(ok, **kw)), 8)


# ------------------------------------------------------------------------------------------------ (h) it helps
def test_optimised_gains_beat_a_sluggish_scalar():
    """(h) 10x10, 16 environments, scalar gain 0.2, grid 0 .. 1 in 15 values plus 0.2.  512 open-loop frames; the float64
    statement on them predicts rho = sum J(opt) / sum J(0.2) (rho > 0.9: ill-posed, the test FAILS).  Then 512
    closed-loop frames on the same seeds with the scalar and with the optimised pooled gains: the measured ratio of
    sum_m mean(e^2) must be <= 1 - (1 - rho) / 2 -- at least half the predicted improvement; the other half is the
    allowance for the sensor's non-linearity and the open-loop transient, which the linear model does not carry.
    (Measured on an MI355X: rho 0.2859, ratio 0.2804, bound 0.6429; LAB_NOTEBOOK.md.)"""
    nrec, nskip = 512, 50
    env = _env(16)
    sup, sim = env.supervisor, env.supervisor.sim
    sup.set_gain(0.2)
    grid = np.concatenate([mg.gain_grid(0.0, 1.0, 15), [0.2]])
    opt = mg.ModalGainOptimizer(sup, grid, nskip=nskip, native=True)
    assert opt.gains.size == 16
    x = mg.record_open_loop(sup, nrec)                                   # the series itself, for the statement
    J, G, st = opt.run(nrec, pool="all")
    assert opt.frames == nrec and G.shape == (sup.nmodes,)
    Jr = mg.loop_rejection(x.cpu().numpy(), opt.gains, sup.s.delay, nskip=nskip)
    keep = mg.pole_radius(opt.gains, sup.s.delay) <= 0.99
    np.testing.assert_allclose(J[..., keep], Jr[..., keep], rtol=1e-9)   # same seeds, same frames: the same series
    Jp = Jr.sum(axis=0)
    i02 = int(np.flatnonzero(opt.gains == np.float64(np.float32(0.2)))[0])
    best = mg.argmin_gain(Jp, opt.gains, st)
    assert (best == opt.index).all() and st[best].all()
    rho = float(Jp[np.arange(sup.nmodes), best].sum() / Jp[:, i02].sum())
    assert rho <= 0.9, "ill-posed: the statement predicts rho = %.3f" % rho

    def closed_loop():
        sup.reset()
        acc = torch.zeros(16, sup.nmodes, dtype=torch.float64, device="cuda:0")
        for t in range(nrec):
            sup.next_part_two(None, linear_control=True)
            sup.next_part_one()
            if t >= nskip:
                acc += sim.slopes2modes().double() ** 2
        return float(acc.sum().item())
    scalar = closed_loop()
    mgain = opt.apply()
    assert np.allclose(mgain * 0.2, G, rtol=1e-6)
    modal = closed_loop()
    ratio = modal / scalar
    print("modal gains: predicted rho %.4f, measured ratio %.4f (bound %.4f); G in [%.3f, %.3f]"
          % (rho, ratio, 1 - (1 - rho) / 2, G.min(), G.max()))
    assert ratio <= 1 - (1 - rho) / 2
