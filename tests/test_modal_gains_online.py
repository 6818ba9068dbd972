"""On-line modal gain optimisation (ao_marl_amd/modal_gains.py OnlineLoopBank), CPU side: the float64 statement against
the off-line bank, a case worked by hand, the pseudo-open-loop identity on a synthetic linear loop, pooling order,
smoothing, restart, every refusal, and the host half of the native optimiser (csrc/aomarl_modopti_host.h: the per-frame
schedule and the desc validation) through its stand-alone program under the sanitizers."""
import os
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest

from ao_marl_amd import modal_gains as mg

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ao_marl_amd", "csrc")
NEVER = 10 ** 9


def _series(rng, frames, nenv, nmodes):
    return np.cumsum(rng.standard_normal((frames, nenv, nmodes)), axis=0) * np.linspace(0.1, 1.5, nmodes) + \
        rng.standard_normal((frames, nenv, nmodes))


@pytest.mark.parametrize("delay", (0.0, 1.0, 1.5, 2.0))
def test_without_forgetting_it_is_the_offline_bank(delay):
    """(1) forget = 1, no apply: J is loop_rejection's, bit for bit -- 1.0 * J + e * e is J + e * e in IEEE arithmetic."""
    x = _series(np.random.default_rng(3), 120, 3, 7)
    gains = np.linspace(0.0, 1.2, 7)
    for nskip in (0, 40):
        b = mg.OnlineLoopBank(gains, delay, nskip=nskip, period=NEVER, forget=1.0)
        for row in x:
            assert b.push(row) is False
        assert b.frames == 120 and b.counted == 120 - nskip and b.updates == 0
        assert np.array_equal(b.J, mg.loop_rejection(x, gains, delay, nskip=nskip))


def test_four_frames_by_hand():
    """(2) delay 0 (wa = 1), gains (0, 0.5), nskip 1, forget 0.5, period 2, beta 0.5, G0 0.4, x = 1, 2, 0, -1.
    g = 0.5: eps = 1, 1.5, -1.25, -1.625;  c0 = 0.5, 1.25, 0.625, -0.1875;  J = -, 2.25, 2.6875, 3.984375
    g = 0:   eps = x;                                                       J = -, 4,    2,      2
    apply behind frame 2: argmin (4, 2.25) = 0.5, G = 0.4 + 0.5 (0.5 - 0.4) = 0.45
    apply behind frame 4: argmin (2, 3.984375) = 0, G = 0.45 + 0.5 (0 - 0.45) = 0.225.  Every value is a dyadic rational
    or a single rounding of one: compared exactly."""
    b = mg.OnlineLoopBank([0.0, 0.5], 0.0, nskip=1, period=2, forget=0.5, beta=0.5, pool=None, G0=[[0.4]])
    applied, Js = [], []
    for v in (1.0, 2.0, 0.0, -1.0):
        applied.append(b.push(np.array([[v]])))
        Js.append(b.J[0, 0].copy())
        if len(applied) == 2:
            assert b.G[0, 0] == 0.4 + 0.5 * (0.5 - 0.4) and b.index[0, 0] == 1
    assert applied == [False, True, False, True]
    assert [list(j) for j in Js] == [[0.0, 0.0], [4.0, 2.25], [2.0, 2.6875], [2.0, 3.984375]]
    assert b.c[0][0, 0, 1] == -0.1875 and b.c[1][0, 0, 1] == 0.625 and b.c[2][0, 0, 1] == 1.25
    assert b.index[0, 0] == 0 and b.G[0, 0] == 0.45 + 0.5 * (0.0 - 0.45)
    assert (b.frames, b.since, b.counted, b.updates) == (4, 4, 3, 2)
    assert b.mgain(0.2)[0, 0] == np.float32(b.G[0, 0] / np.float64(np.float32(0.2)))


@pytest.mark.parametrize("delay", (0.0, 1.0, 1.5, 2.0))
def test_pseudo_open_loop_identity(delay):
    """(3) A linear loop in the simulator's call order: frame t applies voltage[t] = delay line of the commands left at
    t-1, t-2, t-3 plus an "agent" term (part of it outside the modal basis), the sensor then measures
    e[t] = a[t] - v2m . voltage[t] of AR(1) modes a, and the integrator runs m[t] = m[t-1] + g[t] (.) e[t] with gains that
    change every frame.  x = e + v2m . voltage is the open-loop series a to 1e-12, whatever made the voltage; without
    the agent p is wa m[t-1] + wb m[t-2] + wc m[t-3] to the modal round trip (v2m . m2v = I to round-off)."""
    rng = np.random.default_rng(11 + int(10 * delay))
    T, nenv, nm, nact = 200, 2, 6, 9
    m2v = rng.standard_normal((nact, nm))
    v2m = np.linalg.pinv(m2v)
    wa, wb, wc = mg.delay_weights(delay)
    for agent_on in (False, True):
        a = np.zeros((nenv, nm))
        m = [np.zeros((nenv, nm))] * 3                       # m[t-1], m[t-2], m[t-3]
        worst = worst_p = 0.0
        for t in range(T):
            a = 0.97 * a + rng.standard_normal((nenv, nm))
            g = 0.1 + 0.3 * rng.random((nenv, nm))
            line = wa * m[0] + wb * m[1] + wc * m[2]
            agent = 0.3 * rng.standard_normal((nenv, nact)) if agent_on else 0.0
            voltage = line @ m2v.T + agent
            p = voltage @ v2m.T
            e = a - p                                        # -s2m . slopes of a sensor that sees the mirror as applied
            m = [m[0] + g * e, m[0], m[1]]
            worst = max(worst, np.abs(e + p - a).max())
            worst_p = max(worst_p, np.abs(p - line).max())
        assert worst <= 1e-12
        if agent_on:
            assert worst_p > 1e-2                            # (the command history alone would miss the agents)
        else:
            assert worst_p <= 1e-12 * max(1.0, np.abs(m[0]).max())


def test_pooling_sums_the_environments_in_ascending_order():
    b = mg.OnlineLoopBank([0.1, 0.2], 1.0, nskip=0, period=NEVER, pool="all")
    b.push(np.zeros((3, 2)))
    b.J = np.array([1.0, 1e16, -1e16])[:, None, None] * np.ones((3, 2, 2))
    assert (b.pooled() == (1.0 + 1e16) - 1e16).all() and (b.pooled() != 1.0 + (1e16 - 1e16)).all()
    # pooled against per environment: one G per mode / one per environment and mode
    x = _series(np.random.default_rng(5), 64, 3, 4)
    gains = np.linspace(0.0, 0.9, 7)
    pooled = mg.OnlineLoopBank(gains, 1.0, nskip=0, period=64, pool="all")
    each = mg.OnlineLoopBank(gains, 1.0, nskip=0, period=64, pool=None)
    for row in x:
        pooled.push(row)
        each.push(row)
    J = mg.loop_rejection(x, gains, 1.0)
    st = mg.stable(gains, 1.0)
    assert pooled.G.shape == (4,) and each.G.shape == (3, 4) and pooled.updates == each.updates == 1
    assert np.array_equal(pooled.G, gains[mg.argmin_gain((J[0] + J[1]) + J[2], gains, st)])
    assert np.array_equal(each.G, gains[mg.argmin_gain(J, gains, st)])


def test_beta_smooths_towards_the_argmin():
    x = _series(np.random.default_rng(6), 96, 2, 3)
    gains = np.linspace(0.0, 0.9, 10)
    G0 = np.full(3, 0.2)
    hard = mg.OnlineLoopBank(gains, 1.0, nskip=0, period=32, beta=1.0, G0=G0)
    soft = mg.OnlineLoopBank(gains, 1.0, nskip=0, period=32, beta=0.25, G0=G0)
    G = G0.copy()
    for t, row in enumerate(x):
        hard.push(row)
        soft.push(row)
        if (t + 1) % 32 == 0:
            assert np.array_equal(hard.G, gains[hard.index])           # beta = 1: G + (g - G) is g for these operands
            assert np.array_equal(hard.index, soft.index)              # J does not depend on the applies
            G = G + 0.25 * (gains[soft.index] - G)
            assert np.array_equal(soft.G, G)
    assert soft.updates == 3 and np.array_equal(G0, np.full(3, 0.2))   # (the caller's G0 is not written)


def test_restart_keeps_J_and_G():
    x = _series(np.random.default_rng(7), 60, 2, 3)
    gains = np.linspace(0.0, 0.9, 4)
    b = mg.OnlineLoopBank(gains, 1.5, nskip=10, period=25, forget=0.99, pool=None)
    for row in x[:30]:
        b.push(row)
    J, G = b.J.copy(), b.G.copy()
    assert b.updates == 1 and b.counted == 20
    b.restart()
    assert np.array_equal(b.J, J) and np.array_equal(b.G, G) and b.since == 0 and b.frames == 30
    assert all((c == 0).all() for c in b.c)
    for row in x[30:40]:                                     # the new episode's transient: nothing enters J
        b.push(row)
    assert np.array_equal(b.J, J) and b.counted == 20
    # ... and the filters did start from zero: the next frames' J is forget-weighted onto the old one
    fresh = mg.OnlineLoopBank(gains, 1.5, nskip=10, period=NEVER, forget=0.99, pool=None)
    for row in x[30:60]:
        fresh.push(row)
    for row in x[40:60]:
        b.push(row)
    assert b.updates == 2                                    # frame 50: counted over all frames pushed
    np.testing.assert_allclose(b.J, 0.99 ** 20 * J + fresh.J, rtol=1e-12)


def test_refusals_name_the_argument():
    ok = dict(gains=[0.1, 0.3], delay=1.0)
    for kw, word in ((dict(forget=0.0), "forget"), (dict(forget=1.01), "forget"), (dict(forget=-1.0), "forget"),
                     (dict(beta=0.0), "beta"), (dict(beta=1.5), "beta"), (dict(period=0), "period"),
                     (dict(nskip=-1), "nskip"), (dict(pool="some"), "pool"), (dict(delay=2.5), "delay"),
                     (dict(gains=[]), "gains"), (dict(gains=[0.1, float("inf")]), "gains"),
                     (dict(gains=[1.0, 1.5]), "stable"), (dict(gains=[2.5], delay=0.0), "stable")):
        with pytest.raises(ValueError, match=word):
            mg.OnlineLoopBank(**dict(ok, **kw))
    b = mg.OnlineLoopBank(pool="all", G0=np.zeros((2, 3)), **ok)
    with pytest.raises(ValueError, match="G0"):
        b.push(np.zeros((2, 3)))
    b = mg.OnlineLoopBank(**ok)
    b.push(np.zeros((2, 3)))
    with pytest.raises(ValueError, match="the bank"):
        b.push(np.zeros((2, 4)))


def test_supervisor_refusals_name_the_state():
    """modification_online, the denoiser, a prefetched reset and the frame pipeline's twin are refused as
    record_open_loop refuses them; per-environment and zero gains too."""
    def sup(**kw):
        base = dict(sim=NS(_twin=None, nenv=2), s=NS(delay=1.0), reset_prefetch=None, pure_delay_0=False,
                    autoencoder=None, gain=0.4, nmodes=3, online_modal_gains=None)
        base.update(kw)
        return NS(**base)
    for kw, exc, word in ((dict(reset_prefetch="same"), RuntimeError, "reset_prefetch"),
                          (dict(sim=NS(_twin=object(), nenv=2)), RuntimeError, "frame pipeline"),
                          (dict(pure_delay_0=True), NotImplementedError, "modification_online"),
                          (dict(autoencoder=object()), NotImplementedError, "denoiser"),
                          (dict(gain=None), RuntimeError, "per-environment gains"),
                          (dict(gain=0.0), RuntimeError, "gain is 0"),
                          (dict(online_modal_gains=object()), RuntimeError, "already")):
        with pytest.raises(exc, match=word) as info:
            mg.OnlineModalGains(sup(**kw)).start()
        assert "OnlineModalGains.start" in str(info.value)
    with pytest.raises(ValueError, match="pool"):
        mg.OnlineModalGains(sup(), pool="half")
    with pytest.raises(ValueError, match="horizon"):
        mg.OnlineModalGains(sup(), horizon=0)
    assert mg.OnlineModalGains(sup(), horizon=None).forget == 1.0
    assert mg.OnlineModalGains(sup(), horizon=512).forget == float(np.exp(-1.0 / 512))


def test_host_check_builds_and_passes(tmp_path):
    """(5) modopti_online_host_check.cpp under the address and undefined-behaviour sanitizers: the ring schedule against
    a frame-by-frame model (chunks 1..32, periods around the chunk, restarts inside a ring), every refusal of the desc
    validator."""
    exe = str(tmp_path / "modopti_online_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(CSRC, "modopti_online_host_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "modopti_online_host_check: ok"
