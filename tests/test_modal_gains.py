"""Modal gain optimisation (ao_marl_amd/modal_gains.py), CPU side: the float64 statement of the loop-filter bank against
scipy's filter, the stability test against the closed-form limits and against the host half of the native bank
(csrc/aomarl_modopti_host.h through its stand-alone program), the grid, ties, pooling and chunked feeding."""
import os
import subprocess

import numpy as np
import pytest

from ao_marl_amd import modal_gains as mg

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ao_marl_amd", "csrc")
DELAYS = (0.0, 0.5, 1.0, 1.5, 2.0)


def _gains_inside(delay, rmax, n=5):
    """n gains spread over those whose pole radius is at most rmax"""
    cand = np.linspace(0.02, 1.98, 197)
    cand = cand[mg.pole_radius(cand, delay) <= rmax]
    assert cand.size >= n
    return cand[np.linspace(0, cand.size - 1, n).round().astype(int)]


@pytest.mark.parametrize("delay", DELAYS)
def test_statement_is_scipys_filter(delay):
    """(a) loop_rejection against lfilter([1, -1], [1, g wa - 1, g wb, g wc], x): both are the same finite recursion in
    double; with pole radii <= 0.95 round-off is amplified by at most 1 / (1 - 0.95) = 20 -> rtol 1e-10."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(int(10 * delay) + 1)
    x = rng.standard_normal((300, 4, 3))
    gains = _gains_inside(delay, 0.95)
    assert mg.pole_radius(gains, delay).max() <= 0.95
    wa, wb, wc = mg.delay_weights(delay)
    for nskip in (0, 10):
        J = mg.loop_rejection(x, gains, delay, nskip=nskip)
        assert J.shape == (4, 3, 5)
        for j, g in enumerate(gains):
            e = lfilter([1.0, -1.0], [1.0, g * wa - 1.0, g * wb, g * wc], x, axis=0)
            np.testing.assert_allclose(J[..., j], (e[nskip:] ** 2).sum(axis=0), rtol=1e-10, atol=0)


def test_delay_weights_are_the_delay_lines():
    """aomarl_apply_control (aomarl_capi_stages.hip): d <= 1: (1 - d, d, 0); else (0, 2 - d, d - 1)"""
    assert mg.delay_weights(0) == (1.0, 0.0, 0.0) and mg.delay_weights(1) == (0.0, 1.0, 0.0)
    assert mg.delay_weights(0.25) == (0.75, 0.25, 0.0) and mg.delay_weights(1.75) == (0.0, 0.25, 0.75)
    assert mg.delay_weights(2) == (0.0, 0.0, 1.0)
    for bad in (-0.1, 2.01, float("nan")):
        with pytest.raises(ValueError, match="delay"):
            mg.delay_weights(bad)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("modopti") / "modopti_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(CSRC, "modopti_host_check.cpp")])
    return exe


def test_host_check_builds_and_passes(host_check):
    """modopti_host_check.cpp under the address and undefined-behaviour sanitizers: delay weights, closed-form limits,
    Jury's criterion against the loop itself, every refusal of the desc validator."""
    out = subprocess.run([host_check], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "modopti_host_check: ok"


def test_stability_limits(host_check):
    """(b) delay 0: stable iff 0 < g < 2; delay 1: iff g < 1; delay 2: iff g < (sqrt 5 - 1) / 2, at limit x (1 +- 1e-3);
    g = 0 (a marginal pole at 1, cancelled: e = x, no growth) is a legal candidate; numpy.roots and the host header's
    Jury criterion agree, also between the limits and at fractional delays."""
    limits = {0.0: 2.0, 1.0: 1.0, 2.0: 0.5 * (np.sqrt(5.0) - 1.0)}
    for delay, lim in limits.items():
        g = np.array([0.0, 1e-3, lim * (1 - 1e-3), lim * (1 + 1e-3), -1e-3, 0.5 * lim, 3.0])
        want = np.array([True, True, True, False, False, True, False])
        assert (mg.stable(g, delay) == want).all(), delay
        out = subprocess.run([host_check, "stable", repr(delay)] + [repr(float(v)) for v in g], capture_output=True,
                             text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        assert [int(v) for v in out.stdout.split()] == [int(v) for v in want], delay
    # the exactly marginal candidates of the usual grids (poles ON the circle) are not stable, on either side
    for delay, g in ((1.0, 1.0), (0.0, 2.0), (0.5, 2.0)):
        assert not mg.stable(np.array([g]), delay)[0]
        out = subprocess.run([host_check, "stable", repr(delay), repr(g)], capture_output=True, text=True, timeout=60)
        assert out.stdout.split() == ["0"], (delay, g)
    assert not mg.stable(mg.gain_grid(), 1.0)[-1] and mg.stable(mg.gain_grid(), 1.0)[:-1].all()
    grid = np.round(np.linspace(-0.2, 2.2, 49), 6)
    for delay in (0.25, 0.5, 0.75, 1.25, 1.5, 1.75):
        r = mg.pole_radius(grid, delay)
        keep = np.abs(r - 1.0) > 1e-6            # (an exactly marginal root is decided by round-off on either side)
        out = subprocess.run([host_check, "stable", repr(delay)] + [repr(float(v)) for v in grid[keep]],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        assert [bool(int(v)) for v in out.stdout.split()] == list(mg.stable(grid[keep], delay)), delay


def test_gain_grid():
    g = mg.gain_grid()
    assert g.shape == (15,) and g[0] == 0.0 and g[-1] == 1.0 and np.allclose(np.diff(g), 1.0 / 14)
    assert mg.gain_grid(0.1, 0.5, 1).tolist() == [0.1]
    for bad in (dict(ngain=0), dict(gmin=1.0, gmax=0.5), dict(gmax=float("inf"))):
        with pytest.raises(ValueError):
            mg.gain_grid(**bad)


def test_ties_zero_series_and_unstable_candidates():
    """(c) an all-zero series takes the lowest gain; a tie takes the lowest GAIN whatever its index; an unstable candidate
    is never returned, a non-finite J counts as +inf"""
    gains = np.array([0.6, 0.0, 0.3, 1.5])          # 1.5 is unstable at delay 1
    st = mg.stable(gains, 1.0)
    assert st.tolist() == [True, True, True, False]
    J = mg.loop_rejection(np.zeros((40, 2)), gains, 1.0)
    assert (J == 0).all() and mg.argmin_gain(J, gains, st).tolist() == [1, 1]
    J = np.array([[2.0, 3.0, 2.0, 1.0], [np.nan, np.inf, 5.0, 0.0], [np.inf, np.inf, np.inf, 0.0]])
    assert mg.argmin_gain(J, gains, st).tolist() == [2, 2, 1]
    assert mg.argmin_gain(J, gains, np.zeros(4, bool)).tolist() == [-1, -1, -1]
    rng = np.random.default_rng(3)
    bank = mg.LoopBank(gains, 1.0).accumulate(rng.standard_normal((200, 6)))
    J, arg, st = bank.result()
    assert np.isfinite(J[:, :3]).all() and (arg != 3).all()


def test_pooling_nskip_and_chunks():
    """(c) the pooled argmin is the argmin of the summed J; nskip is honoured; feeding halves gives the whole"""
    rng = np.random.default_rng(11)
    T, nenv, nm = 120, 4, 6
    # a random walk per series (atmosphere-like: some gain helps), with a different step size per mode
    x = np.cumsum(rng.standard_normal((T, nenv, nm)), axis=0) * np.linspace(0.2, 2.0, nm) + rng.standard_normal((T, nenv, nm))
    gains = np.unique(mg.gain_grid().astype(np.float32)).astype(np.float64)
    J = mg.loop_rejection(x, gains, 1.0, nskip=20)
    st = mg.stable(gains, 1.0)
    pooled = mg.argmin_gain(J.sum(axis=0), gains, st)
    assert pooled.shape == (nm,) and (pooled == np.argmin(np.where(st, J.sum(axis=0), np.inf), axis=-1)).all()
    assert (pooled > 0).all()                         # a random walk is better tracked than left alone
    # nskip: the frames before it do not count, the filter runs through them all the same
    wa, wb, wc = mg.delay_weights(1.0)
    g = gains[5]
    c, e = np.zeros((4,) + x.shape[1:]), np.zeros_like(x)
    for t in range(T):
        e[t] = x[t] - (wa * c[0] + wb * c[1] + wc * c[2])
        c = np.concatenate([(c[0] + g * e[t])[None], c[:3]])
    np.testing.assert_allclose(J[..., 5], (e[20:] ** 2).sum(axis=0), rtol=1e-12)
    np.testing.assert_allclose(mg.loop_rejection(x, gains, 1.0, nskip=0)[..., 5], (e ** 2).sum(axis=0), rtol=1e-12)
    assert (mg.loop_rejection(x, gains, 1.0, nskip=T) == 0).all()
    # halves equal the whole, bit for bit
    for cut in (1, 19, 20, 21, 60):
        b = mg.LoopBank(gains, 1.0, nskip=20).accumulate(x[:cut]).accumulate(x[cut:])
        assert b.frames == T and np.array_equal(b.J, J), cut
    # one grid per series (what the closed-loop identity test uses)
    per = np.stack([gains[[2, 5, 9]]] * nm)
    Jp = mg.loop_rejection(x, per, 1.0, nskip=20)
    assert np.array_equal(Jp, J[..., [2, 5, 9]])


def test_optimizer_needs_a_scalar_gain():
    """apply() refuses a supervisor without one scalar gain, and a gain of 0"""
    from types import SimpleNamespace as NS
    sup = NS(s=NS(delay=1.0), gain=None)
    opt = mg.ModalGainOptimizer(sup, native=False)
    with pytest.raises(RuntimeError, match="run"):
        opt.apply()
    opt.G = np.full(4, 0.5)
    with pytest.raises(RuntimeError, match="per-environment"):
        opt.apply()
    sup.gain = 0.0
    with pytest.raises(RuntimeError, match="gain is 0"):
        opt.apply()
    got = []
    sup.gain, sup.set_modal_gains = 0.25, got.append
    assert opt.apply().tolist() == [2.0] * 4 and got[0].dtype == np.float32


def test_roket_refuses_a_modal_law():
    """(g) VecRoket's loop filter gRD assumes the scalar law: a supervisor with modal gains is refused, by name"""
    from types import SimpleNamespace as NS
    from ao_marl_amd import params, roket
    sim = NS(_twin=None, prefetch=False, pending_atmos=False)
    sup = NS(sim=sim, prefetch_atmos=False, reset_prefetch=None, gain=0.7, _env_gains=False, geo=object(),
             pure_delay_0=False, autoencoder=None, config=params.builtin("production_sh_10x10_2m"), modal_gains=None)
    env = NS(supervisor=sup, frame_pipeline=False, rl_step=lambda *a, **k: None)
    assert roket._roket_supervisor(env) is sup
    sup.modal_gains = np.ones((1, 85), dtype=np.float32)
    with pytest.raises(RuntimeError, match="set_modal_gains"):
        roket._roket_supervisor(env)


def test_controller_parameters_reach_the_system_description():
    """modopti, nrec, gmin, gmax, ngain of the controller (PCONTROLLER.py:78-88) are read; nothing acts on them by itself"""
    from ao_marl_amd import params
    c = params.Param_controller()
    assert (c.modopti, c.nrec, c.gmin, c.gmax, c.ngain) == (False, 2048, 0.0, 1.0, 15)
    from tests import helpers
    _, s, _ = helpers.calibrated("production_sh_10x10_2m")
    assert (s.modopti, s.nrec, s.gmin, s.gmax, s.ngain) == (False, 2048, 0.0, 1.0, 15)
