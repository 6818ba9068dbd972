"""On-line modal gain optimisation on the GPU: the native on-line bank (aomarl_modopti_online_*) against its float64
statement (modal_gains.OnlineLoopBank) through push, the hook in aomarl_do_control (pseudo-open-loop modes in the ring,
the applies that write the context's gains), attach -> detach against a context that never had an optimiser, and the
closed loop against the off-line optimum: stationary, and tracking a change of wind."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import libaomarl as la  # noqa: E402
from ao_marl_amd import modal_gains as mg  # noqa: E402

NAME = "production_sh_10x10_2m"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
NEVER = 2 ** 31 - 1
FRAMES = 100          # 3 LDS tiles of 32 frames and a remainder


def _grid(ngain):
    # 7: up to 1.2; 33: up to 2.2 (two gain passes of the bank) -- unstable candidates at every delay
    return {7: np.linspace(0.0, 1.2, 7), 33: np.linspace(0.0, 2.2, 33)}[ngain]


def _series(rng, nenv, nmodes):
    """the generator of test_bank_is_the_float64_statement: a random walk, a different mix per mode, plus white noise"""
    x = np.cumsum(rng.standard_normal((FRAMES, nenv, nmodes)), axis=0) * np.linspace(0.1, 1.5, nmodes) + \
        rng.standard_normal((FRAMES, nenv, nmodes))
    return np.ascontiguousarray(x, dtype=np.float32)


def _near_tie(Jp, st):
    """entries whose two best stable J lie within 1e-8 relative (exact ties go by the tie rule on both sides)"""
    Js = np.sort(np.where(st, np.where(np.isfinite(Jp), Jp, np.inf), np.inf), axis=-1)
    if st.sum() < 2:
        return np.zeros(Js.shape[:-1], bool)
    gap = (Js[..., 1] - Js[..., 0]) / np.maximum(Js[..., 1], 1e-300)
    return (Js[..., 1] != Js[..., 0]) & (gap <= 1e-8)


# ------------------------------------------------------------------------------------------------ (a) the bank
@pytest.mark.parametrize("delay", (0.0, 1.0, 1.5, 2.0))
def test_online_bank_is_the_float64_statement(delay):
    """(a) through push, 3 environments, 100 frames: nmodes 5 / 64 / 87, grids of 7 and 33 candidates, nskip 0 / 40,
    forget 1 / 0.98 (beta 1 / 0.5), period 31 / 32 / 33, pooled and not, chunk 1 / 32.  J at rtol 1e-9 for candidates of
    pole radius <= 0.99 (100 frames x 1.1e-16 x the amplification 1 / (1 - 0.99), FMA contraction being the only
    difference; the forgetting factor only shrinks old terms); G after every apply equal to the statement's, entries
    whose two best stable J lie within 1e-8 relative (at that or an earlier apply) left out, at most 0.1 % of them;
    chunk 1 against chunk 32 and two runs bit-identical; forget = 1 without an apply: J is NativeLoopBank's bits."""
    nenv, total, left_out = 3, 0, 0
    rng = np.random.default_rng(200 + int(10 * delay))
    for nmodes in (5, 64, 87):
        x32 = _series(rng, nenv, nmodes)
        xd = torch.as_tensor(x32, device="cuda:0")
        for ngain in (7, 33):
            for nskip in (0, 40):
                off = mg.NativeLoopBank(nenv, nmodes, _grid(ngain), delay, nskip).accumulate(xd)
                Joff = off.result()[0]
                for chunk in (1, 32):
                    b = mg.NativeOnlineLoopBank(nenv, nmodes, _grid(ngain), delay, nskip, NEVER, 1.0, 1.0, "all", None, chunk=chunk)
                    for t in range(FRAMES):
                        b.push(xd[t])
                    J, arg, G, _, counts = b.result()
                    assert np.array_equal(J, Joff), (nmodes, ngain, nskip, chunk)
                    assert counts == dict(frames=FRAMES, since=FRAMES, counted=FRAMES - nskip, updates=0)
                    assert (arg == -1).all() and (G == 0).all()
                for forget in (1.0, 0.98):
                    beta = 1.0 if forget == 1.0 else 0.5
                    for period in (31, 32, 33):
                        for pool in ("all", None):
                            G0 = rng.random(nmodes if pool == "all" else (nenv, nmodes))
                            run = {}
                            for key, chunk in (("c1", 1), ("c32", 32), ("again", 32 if period == 32 else None)):
                                if chunk is None:
                                    continue
                                b = mg.NativeOnlineLoopBank(nenv, nmodes, _grid(ngain), delay, nskip, period, forget, beta,
                                                            pool, G0, chunk=chunk)
                                Gs = []
                                for t in range(FRAMES):
                                    b.push(xd[t])
                                    if (t + 1) % period == 0 and t >= nskip:
                                        Gs.append(b.result()[2])
                                run[key] = (b.result(), Gs)
                                gains = b.gains
                            (J, arg, G, st, counts), Gs = run["c1"]
                            for other in ("c32", "again"):
                                if other in run:
                                    (J2, arg2, G2, _, counts2), Gs2 = run[other]
                                    assert np.array_equal(J, J2) and np.array_equal(arg, arg2) and np.array_equal(G, G2)
                                    assert counts == counts2 and len(Gs) == len(Gs2)
                                    assert all(np.array_equal(a, c) for a, c in zip(Gs, Gs2)), (period, pool, other)
                            ref = mg.OnlineLoopBank(gains, delay, nskip, period, forget, beta, pool, G0)
                            assert (st == ref.stable).all()
                            out = np.zeros(G.shape, bool)
                            k = 0
                            for t in range(FRAMES):
                                if ref.push(x32[t]):
                                    out |= _near_tie(ref.pooled(), st).reshape(out.shape)
                                    got = Gs[k].reshape(out.shape)
                                    want = ref.G.reshape(out.shape)
                                    assert np.array_equal(got[~out], want[~out]), (nmodes, ngain, nskip, forget, period, pool, k)
                                    total += out.size
                                    left_out += int(out.sum())
                                    k += 1
                            assert k == len(Gs) == ref.updates == counts["updates"]
                            assert counts == dict(frames=ref.frames, since=ref.since, counted=ref.counted, updates=ref.updates)
                            assert np.array_equal(arg.reshape(out.shape)[~out], ref.index.reshape(out.shape)[~out])
                            ok = (mg.pole_radius(gains, delay) <= 0.99) | (gains == 0.0)
                            np.testing.assert_allclose(J[..., ok], ref.J[..., ok], rtol=1e-9, atol=0)
    print("on-line bank, delay %g: %d of %d G entries left out as near-ties" % (delay, left_out, total))
    assert total == 4 * 9360 and left_out <= 0.001 * total      # (149 760 over the four delays)


def test_restart_and_refusals():
    """restart() inside a ring: the waiting rows are consumed with the old history, the filters start from zero, J and G
    stay (the statement's restart()), chunk 1 and 32 agree bit for bit; every refusal of create names its field."""
    rng = np.random.default_rng(9)
    x32 = _series(rng, 3, 70)
    xd = torch.as_tensor(x32, device="cuda:0")
    gains = _grid(7)
    res = []
    for chunk in (1, 32):
        b = mg.NativeOnlineLoopBank(3, 70, gains, 1.0, 10, 25, 0.99, 0.5, None, None, chunk=chunk)
        for t in range(FRAMES):
            if t in (45, 77):
                b.restart()
            b.push(xd[t])
        res.append(b.result())
    ref = mg.OnlineLoopBank(b.gains, 1.0, 10, 25, 0.99, 0.5, None)
    for t in range(FRAMES):
        if t in (45, 77):
            ref.restart()
        ref.push(x32[t])
    for a, c in zip(res[0], res[1]):
        assert np.array_equal(a, c) if isinstance(a, np.ndarray) else a == c
    J, arg, G, st, counts = res[0]
    assert counts == dict(frames=100, since=23, counted=ref.counted, updates=4) and ref.updates == 4
    ok = mg.pole_radius(b.gains, 1.0) <= 0.99
    np.testing.assert_allclose(J[..., ok], ref.J[..., ok], rtol=1e-9)
    near = _near_tie(ref.pooled(), st)
    assert near.sum() <= 2 and np.array_equal(arg[~near], ref.index[~near])
    for kw, word in ((dict(forget=0.0), "forget"), (dict(forget=1.5), "forget"), (dict(beta=0.0), "beta"),
                     (dict(beta=2.0), "beta"), (dict(period=0), "period"), (dict(chunk=0), "chunk"), (dict(chunk=33), "chunk"),
                     (dict(nskip=-1), "nskip"), (dict(delay=2.5), "delay"), (dict(gains=[]), "ngain"), (dict(nenv=0), "nenv"),
                     (dict(gains=[1.0, 1.5]), "stable"), (dict(gains=[0.1, float("nan")]), r"gains\[1\]")):
        a = dict(nenv=2, nmodes=4, gains=[0.1, 0.2], delay=1.0, nskip=0, period=8, forget=1.0, beta=1.0, pool="all", chunk=4)
        a.update(kw)
        with pytest.raises(la.AomarlError, match=word):
            mg.NativeOnlineLoopBank(**a)
    with pytest.raises(ValueError, match="pool"):
        mg.NativeOnlineLoopBank(2, 4, [0.1], 1.0, pool="some")
    with pytest.raises(ValueError, match="G0"):
        mg.NativeOnlineLoopBank(2, 4, [0.1], 1.0, pool="all", G0=np.zeros((2, 4)))
    b = mg.NativeOnlineLoopBank(2, 4, [0.1], 1.0)
    with pytest.raises(ValueError):
        b.push(torch.zeros(2, 5, device="cuda:0"))


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


GAIN = 0.4        # gain * mgain in [0.12, 0.48]: stable at delay 1 (< 1) and at delay 2 (< 0.618)


# ------------------------------------------------------------------------------------------------ (b) the hook
@pytest.mark.parametrize("delay", [None, 2.0])
@pytest.mark.parametrize("by_env_step", [False, True])
@pytest.mark.parametrize("pool", ["all", None])
def test_hook_feeds_the_ring_and_applies_the_gains(delay, by_env_step, pool):
    """(b) 64 closed-loop frames of 3 environments from a non-uniform mgain, chunk 1, period 16, beta 1, nskip 0:
    (i)   the ring's row is slopes2modes() + volts2modes(voltage) of the frame to 1e-6 max|x| (the same products;
          fp32 sums of the same operands);
    (ii)  it is E + wa M[t-1] + wb M[t-2] + wc M[t-3] to 2 x 2e-5 max|m|: the modal round trip, once per product;
    (iii) the context's mgain read back behind frame t is float32(G / gain) of the statement run on those ring rows
          (near-ties of 1e-8 left out), and do_control of frame t + 1 uses it: m[t+1] - m[t] = gain * mgain (.) e[t+1] to
          2e-5 max|m|, (i) of test_law_and_bank_are_the_same_recursion, while the gains the run started with miss it."""
    T = 64
    env = _env(3, delay)
    sup, sim = env.supervisor, env.supervisor.sim
    nm = sup.nmodes
    rows = 1 if pool == "all" else 3
    mgain0 = _mgain(nm, None if pool == "all" else 3).reshape(rows, nm)
    sup.set_gain(GAIN)
    sup.set_modal_gains(mgain0)
    grid = np.linspace(0.0, 0.6, 7)
    opt = mg.OnlineModalGains(sup, grid, nskip=0, period=16, beta=1.0, pool=pool, chunk=1).start()
    assert sup.online_modal_gains is opt
    with pytest.raises(la.AomarlError, match="on-line optimiser is attached"):
        sup.set_modal_gains(mgain0)
    gain32 = np.float64(np.float32(GAIN))
    ref = mg.OnlineLoopBank(opt.gains, opt.delay, 0, 16, 1.0, 1.0, pool, (gain32 * mgain0.astype(np.float64)).reshape(
        nm if pool == "all" else (3, nm)))
    zero = torch.zeros(env.nenv, env.action_dim, device="cuda:0")
    if by_env_step:
        env.reset()                                   # frame 0: linear_step
    else:
        sup.reset()
    E, M, X, XP, MG = [], [], [], [], []
    out = np.zeros((rows, nm), bool)
    for t in range(T):
        if by_env_step:
            if t:
                env.step(zero)
                assert env._glue is not None
            E.append(env._res_modes.double().cpu().numpy())
            M.append(sim.volts2modes(sup.get_command()).double().cpu().numpy())
        else:
            sup.next_part_two(None, linear_control=True)
            sup.next_part_one()
            E.append(sim.slopes2modes().double().cpu().numpy())
            M.append(sim.volts2modes(sim.com).double().cpu().numpy())
        X.append(opt.bank.last().cpu().numpy())
        XP.append((sim.slopes2modes().double() + sim.volts2modes(sim.voltage).double()).cpu().numpy())
        if ref.push(X[-1]):
            out |= _near_tie(ref.pooled(), ref.stable).reshape(rows, nm)
        MG.append(sup.modal_gains.copy())
        want = ref.mgain(GAIN).reshape(rows, nm) if ref.updates else mgain0
        assert np.array_equal(MG[-1][~out], want[~out]), t
    E, M, X, XP, MG = np.stack(E), np.stack(M), np.stack(X).astype(np.float64), np.stack(XP), np.stack(MG)
    assert ref.updates == 4 == opt.updates and out.sum() <= 1
    assert np.abs(MG[-1] - mgain0).max() > 0.05          # the applies did move the gains
    xs, ms = np.abs(X).max(), np.abs(M).max()
    d1 = np.abs(X - XP).max()
    wa, wb, wc = mg.delay_weights(sup.s.delay)
    Z = np.zeros_like(M[:1])
    xm = E + wa * np.concatenate([Z, M[:-1]]) + wb * np.concatenate([Z, Z, M[:-2]]) + wc * np.concatenate([Z, Z, Z, M[:-3]])
    d2 = np.abs(X - xm).max()
    print("ring row: |x - (e + p)| %.3g of max|x| %.3g; |x - (E + delay line)| %.3g of max|m| %.3g" % (d1, xs, d2, ms))
    assert xs > 0 and d1 <= 1e-6 * xs
    assert d2 <= 2 * 2e-5 * ms
    # the law, with the gains read back behind the frame before
    used = np.concatenate([mgain0[None], MG[:-1]])
    g = (np.float32(GAIN) * np.broadcast_to(used, (T, 3, nm)).astype(np.float32)).astype(np.float64)
    Mprev = np.concatenate([Z, M[:-1]])
    dev = np.abs(M - Mprev - g * E).max()
    stale = np.abs(M - Mprev - np.float64(np.float32(GAIN)) * mgain0.astype(np.float64) * E).max()
    print("law under changing gains: max deviation %.3g (the first gains throughout: %.3g) of max|m| %.3g" % (dev, stale, ms))
    assert dev <= 2e-5 * ms
    assert stale > 2e-5 * ms
    # detached: the gains stay as last applied, host copy included; the entry points are free again
    last = MG[-1]
    opt.stop()
    assert sup.online_modal_gains is None and np.array_equal(sup.modal_gains, last)
    assert np.array_equal(opt.G.reshape(rows, nm)[~out], ref.G.reshape(rows, nm)[~out]) and opt.updates == 4
    sup.set_modal_gains(mgain0)


def test_attach_refusals():
    """attach without modal gains, with a row count that does not fit the pooling, with per-environment scalar gains, a
    gain of zero, other sizes; do_control on a partial range of the attached state; a second attach; destroy while
    attached: each refused by name, and the context works on afterwards."""
    env = _env(3)
    sup, sim = env.supervisor, env.supervisor.sim
    nm = sup.nmodes
    sup.set_gain(GAIN)
    sup.ensure_slopes2modes()
    lib = sim.lib

    def bank(nenv=3, nmodes=nm, pool="all"):
        return mg.NativeOnlineLoopBank(nenv, nmodes, [0.1, 0.3], 1.0, pool=pool, chunk=4)
    with pytest.raises(la.AomarlError, match="no modal gains"):
        bank().attach(sim)
    sup.set_modal_gains(_mgain(nm, 3))
    with pytest.raises(la.AomarlError, match="mgain_rows = 3"):
        bank().attach(sim)
    sup.set_modal_gains(_mgain(nm))
    with pytest.raises(la.AomarlError, match="mgain_rows = 1"):
        bank(pool=None).attach(sim)
    with pytest.raises(la.AomarlError, match="nmodes"):
        bank(nmodes=nm + 1).attach(sim)
    with pytest.raises(la.AomarlError, match="nenv = 2"):
        bank(nenv=2).attach(sim)
    sup.set_gain(np.full(3, 0.3, dtype=np.float32))
    with pytest.raises(la.AomarlError, match="per-environment scalar gains"):
        bank().attach(sim)
    sup.set_gain(0.0)
    with pytest.raises(la.AomarlError, match="positive gain"):
        bank().attach(sim)
    sup.set_gain(GAIN)
    b = bank()
    b.attach(sim)
    with pytest.raises(la.AomarlError, match="attached already"):
        bank().attach(sim)
    assert lib.aomarl_modopti_online_destroy(b.ptr) != 0 and b"attached" in lib.aomarl_last_error()
    with pytest.raises(la.AomarlError, match="aomarl_do_control feeds it"):
        b.push(torch.zeros(3, nm, device="cuda:0"))
    sup.reset()
    sup.next_part_two(None, linear_control=True)
    sup.next_part_one(do_control=False)
    with pytest.raises(la.AomarlError, match="partial environment range"):
        sim.do_control(1, 2)
    sim.do_control()
    sim.set_gain(0.0)                                   # err alone: not a frame of the loop
    sim.do_control()
    sim.set_gain(GAIN)
    assert b.result()[4]["frames"] == 1
    b.detach()
    sim.do_control(1, 2)
    assert b.result()[4]["frames"] == 1


# ------------------------------------------------------------------------------------------------ (c) detach
def test_detached_is_a_context_that_never_had_one():
    """(c) an optimiser attached for 20 frames (period beyond them: the gains stay the ones set), then detached: a 12-step
    env_step rollout from reset is bit for bit that of an environment that never had one, and so are the launch
    counters of a step."""
    a, b = _env(3), _env(3)
    nm = a.supervisor.nmodes
    for e in (a, b):
        e.supervisor.set_gain(GAIN)
        e.supervisor.set_modal_gains(_mgain(nm))
    opt = mg.OnlineModalGains(b.supervisor, nskip=0, period=1000, pool="all").start()
    b.reset()
    zero = torch.zeros(3, b.action_dim, device="cuda:0")
    for _ in range(20):
        b.step(zero)
    assert opt.updates == 0 and opt.bank.result()[4]["frames"] == 21
    opt.stop()
    assert np.array_equal(b.supervisor.modal_gains, a.supervisor.modal_gains)
    sa, sb = a.reset(), b.reset()
    assert torch.equal(sa, sb)
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    for it in range(12):
        act = torch.rand(3, a.action_dim, device="cuda:0", generator=gen) * 2 - 1
        if it == 11:
            la.arith_launches(reset=True)
        sa, ra, _, _ = a.step(act)
        if it == 11:
            na = la.arith_launches()
            la.arith_launches(reset=True)
        sb, rb, _, _ = b.step(act)
        if it == 11:
            nb = la.arith_launches()
        assert torch.equal(sa, sb) and torch.equal(ra, rb), it
        assert torch.equal(a.supervisor.sim.strehl, b.supervisor.sim.strehl), it
        assert torch.equal(a.supervisor.sim.com, b.supervisor.sim.com), it
    assert na == nb


# ------------------------------------------------------------------------------------------------ (d), (e) it helps
def _closed_loop(sup, nframes):
    for _ in range(nframes):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()


def _snap(G, gains):
    return np.abs(np.asarray(G)[..., None] - gains).argmin(axis=-1)


def _offline(sup, grid, nrec, nskip):
    """the off-line bank on record_open_loop of the supervisor's seeds: pooled J [nmodes][ngain], gains, stable mask"""
    off = mg.ModalGainOptimizer(sup, grid, nskip=nskip, native=True)
    J, _, st = off.run(nrec, pool="all")
    return J.sum(axis=0), off.gains, st


def _cost(Jp, idx):
    return float(Jp[np.arange(Jp.shape[0]), idx].sum())


def test_stationary_reaches_half_the_offline_improvement():
    """(d) 10x10, 4 environments, scalar gain 0.2 (the "sluggish" case), grid 0 .. 1 in 15 values plus 0.2, pooled, period
    256, no forgetting, 1500 closed-loop frames from the scalar law.  J_off is the off-line bank's pooled J on
    record_open_loop of the same seeds.  With G_on snapped to the nearest candidate:
        sum_m J_off[m][G_on[m]] <= J_off(scalar) - 1/2 (J_off(scalar) - sum_m min_j J_off[m][j])
    -- at least half the improvement the off-line optimum predicts.  (Measured on an MI355X: scalar 135.4, optimum 38.39,
    on-line 38.39: fraction 1.000; LAB_NOTEBOOK.md.)"""
    nframes, nskip = 1500, 50
    env = _env(4)
    sup = env.supervisor
    sup.set_gain(0.2)
    grid = np.concatenate([mg.gain_grid(0.0, 1.0, 15), [0.2]])
    Jp, gains, st = _offline(sup, grid, nframes, nskip)
    i02 = int(np.flatnonzero(gains == np.float64(np.float32(0.2)))[0])
    on = mg.OnlineModalGains(sup, grid, nskip=nskip, period=256, pool="all").start()
    assert np.array_equal(sup.modal_gains, np.ones((1, sup.nmodes), dtype=np.float32))
    sup.reset()
    _closed_loop(sup, nframes)
    G, nup = on.G, on.updates
    on.stop()
    assert nup == nframes // 256 and G.shape == (sup.nmodes,)
    idx = _snap(G, gains)
    assert st[idx].all()
    scalar, best = _cost(Jp, np.full(sup.nmodes, i02)), _cost(Jp, mg.argmin_gain(Jp, gains, st))
    got = _cost(Jp, idx)
    assert scalar > best
    print("on-line, stationary: J_off scalar %.4g, optimum %.4g, on-line gains %.4g: fraction of the predicted "
          "improvement %.3f; G in [%.3f, %.3f]" % (scalar, best, got, (scalar - got) / (scalar - best), G.min(), G.max()))
    assert got <= scalar - 0.5 * (scalar - best)


FAST_WIND = 80.0      # m/s (the builtin's layer moves at 20)


def test_tracks_a_change_of_wind():
    """(e) as (d) with horizon = 512, then atmos.set_wind to FAST_WIND behind the episode and 2000 more frames (the
    optimiser goes on: J and G carry across the reset and are forgotten at exp(-1/512) per frame).  On the open-loop
    record of the NEW wind the stale gains -- what the optimiser held when the wind changed -- must cost at least 1.2 x
    the new optimum (a precondition: the test FAILS when the wind does not make the case), and the gains at the end meet
    the half-improvement condition with the stale gains as the baseline.  (Measured on an MI355X: stale 811.3, optimum
    390.4 -- 2.078 x --, tracked 390.8: fraction 0.999; winds of 40 / 60 / 120 m/s give 1.77 / 2.03 / 2.52 x; LAB_NOTEBOOK.md.)"""
    nskip = 50
    env = _env(4)
    sup = env.supervisor
    sup.set_gain(0.2)
    grid = np.concatenate([mg.gain_grid(0.0, 1.0, 15), [0.2]])
    on = mg.OnlineModalGains(sup, grid, nskip=nskip, period=256, horizon=512, pool="all").start()
    sup.reset()
    _closed_loop(sup, 1500)
    G_stale = on.G.copy()
    sup.atmos.set_wind(0, windspeed=FAST_WIND)
    sup.reset()
    _closed_loop(sup, 2000)
    G, nup = on.G, on.updates
    on.stop()
    assert nup == 3500 // 256
    Jp, gains, st = _offline(sup, grid, 2000, nskip)          # (reset inside: the new wind, the same seeds)
    stale, got, best = _cost(Jp, _snap(G_stale, gains)), _cost(Jp, _snap(G, gains)), _cost(Jp, mg.argmin_gain(Jp, gains, st))
    print("on-line, wind 20 -> %g m/s: J_off stale %.4g, optimum %.4g (stale / optimum %.3f), tracked %.4g: fraction of "
          "the improvement %.3f" % (FAST_WIND, stale, best, stale / best, got, (stale - got) / max(stale - best, 1e-300)))
    assert stale >= 1.2 * best, "the wind does not make the case: stale / optimum = %.3f" % (stale / best)
    assert got <= stale - 0.5 * (stale - best)
