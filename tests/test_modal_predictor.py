"""The modal predictor's float64 statement (predictive.PredictorBank) on the CPU: the ridge identity at forget = 1, two
series worked by hand, the trace cap under forgetting, splits / restart / freeze, that it beats the best integrator on
a predictable series, and the host half of the native code under the sanitizers (predictor_host_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from ao_marl_amd import modal_gains as mg
from ao_marl_amd import predictive as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ao_marl_amd", "csrc")


def _ar2(T, nseries, seed=1):
    """x[t] = 1.95 x[t-1] - 0.951 x[t-2] + 0.02 nu, plus white noise of 0.05: a slow, predictable series"""
    rng = np.random.default_rng(seed)
    nu = rng.standard_normal((T, nseries))
    white = rng.standard_normal((T, nseries))
    a = np.zeros((T, nseries))
    for t in range(T):
        a[t] = 1.95 * (a[t - 1] if t >= 1 else 0.0) - 0.951 * (a[t - 2] if t >= 2 else 0.0) + 0.02 * nu[t]
    return a + 0.05 * white


X = _ar2(4000, 6)


def _normal_equations(x, n, delay, p0, first):
    """(A, b) of the ridge problem over frames >= first: A = sum phi phi^T + I / p0, b = sum phi x + theta0 / p0"""
    wa, wb, wc = mg.delay_weights(delay)
    T, S = x.shape
    xz = np.concatenate([np.zeros((n + 2, S)), x])             # xz[t + n + 2] = x[t]; zero before frame 0

    def h(s):                                                  # [S, n]: x[s], x[s-1], ...
        return np.stack([xz[s + n + 2 - i] for i in range(n)], axis=1)
    A = np.broadcast_to(np.eye(n) / p0, (S, n, n)).copy()
    b = np.zeros((S, n))
    b[:, 0] = 1.0 / p0
    for t in range(first, T):
        phi = wa * h(t - 1) + wb * h(t - 2) + wc * h(t - 3)
        A += phi[:, :, None] * phi[:, None, :]
        b += phi * x[t][:, None]
    return A, b


@pytest.mark.parametrize("order", (1, 4, 8))
def test_ridge_identity(order):
    """forget = 1, p0 = 100: theta is the solution of the normal equations over the learned frames and P the inverse of
    their matrix, to 1e-9 of each array's maximum, at delays 0, 0.4, 1, 1.6, 2"""
    for delay in (0.0, 0.4, 1.0, 1.6, 2.0):
        bank = pc.PredictorBank(order, delay, 1.0, 100.0, 0)
        bank.push(X)
        assert bank.counts == dict(frames=4000, since=4000, learned=4000 - order - 2)
        A, b = _normal_equations(X, order, delay, 100.0, order + 2)
        theta = np.linalg.solve(A, b[:, :, None])[:, :, 0]
        Pinv = np.linalg.inv(A)
        dt = np.abs(bank.theta - theta).max() / np.abs(theta).max()
        dP = np.abs(bank.P - Pinv).max() / np.abs(Pinv).max()
        print("order %d delay %g: theta %.3g, P %.3g of the maximum" % (order, delay, dt, dP))
        assert dt <= 1e-9 and dP <= 1e-9
        assert np.array_equal(bank.P, np.swapaxes(bank.P, -1, -2))


def test_by_hand():
    """x[t] = r^t, order 1, delay 1: phi[t] = x[t-2], learned from frame 3, so with S = sum_{t=3}^{T-1} r^(2 (t-2))
        theta = (1 / p0 + r^2 S) / (1 / p0 + S)   -> r^2
    exactly; an all-zero series leaves theta at its start, bit for bit, and commands exactly 0."""
    r, T, p0 = 0.9, 60, 10.0
    x = r ** np.arange(T, dtype=np.float64)
    bank = pc.PredictorBank(1, 1.0, 1.0, p0, 0)
    bank.push(x[:, None])
    k = np.arange(1, T - 2)
    S = float((r ** (2 * k)).sum())
    want = (1.0 / p0 + r * r * S) / (1.0 / p0 + S)
    assert abs(bank.theta[0, 0] - want) <= 1e-12
    assert abs(bank.P[0, 0, 0] - 1.0 / (1.0 / p0 + S)) <= 1e-12
    assert abs(want - r * r) < 0.02
    for order in (1, 3, 8):
        z = pc.PredictorBank(order, 1.6, 0.99, 1e4, 0)
        c = z.push(np.zeros((50, 2)))
        start = np.zeros((2, order))
        start[:, 0] = 1.0
        assert z.theta.tobytes() == start.tobytes()
        assert c.dtype == np.float32 and (c == 0).all() and not np.signbit(c).any()


@pytest.mark.parametrize("order", (1, 4))
def test_cap(order):
    """forget = 0.98 on an all-zero and on a constant series, 20 000 frames: without excitation P / forget would grow
    without bound; the cap keeps trace(P) <= n p0 and everything finite, and the zero series never moves theta"""
    p0 = 1e4
    x = np.zeros((20000, 2))
    x[:, 1] = 0.3
    bank = pc.PredictorBank(order, 1.0, 0.98, p0, 50)
    bank.push(x)
    P, theta = bank.P, bank.theta
    assert np.isfinite(P).all() and np.isfinite(theta).all()
    tr = np.trace(P, axis1=-2, axis2=-1)
    assert (tr <= order * p0 * (1 + 1e-12)).all() and (tr > 0).all()
    start = np.zeros(order)
    start[0] = 1.0
    assert theta[0].tobytes() == start.tobytes()
    assert np.isfinite(bank.J).all() and bank.J[0] == 0.0


def _state(b):
    return [b.theta, b.P, b.J, b.J0]


def test_splits_restart_and_freeze():
    T, n = 300, 4
    x = X[:T]
    one = pc.PredictorBank(n, 1.6, 0.99, 1e4, 20)
    c_one = one.push(x)
    by1 = pc.PredictorBank(n, 1.6, 0.99, 1e4, 20)
    c_by1 = np.concatenate([by1.push(x[t:t + 1]) for t in range(T)])
    two = pc.PredictorBank(n, 1.6, 0.99, 1e4, 20)
    c_two = np.concatenate([two.push(x[:7]), two.push(x[7:])])
    for other, c in ((by1, c_by1), (two, c_two)):
        assert c.tobytes() == c_one.tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_state(one), _state(other)))
        assert other.counts == one.counts
    # restart: the history and the frame counter start over -- no update for n + 2 frames, J is not counted for nskip
    # frames and carries over
    th, P, J = one.theta.copy(), one.P.copy(), one.J.copy()
    one.restart()
    assert one.counts == dict(frames=T, since=0, learned=T - n - 2)
    one.push(X[T:T + n + 2])
    assert one.theta.tobytes() == th.tobytes() and one.P.tobytes() == P.tobytes() and one.J.tobytes() == J.tobytes()
    one.push(X[T + n + 2:T + n + 3])
    assert (one.theta != th).any() and (one.P != P).any() and one.J.tobytes() == J.tobytes()
    one.push(X[T + n + 3:T + 21])
    assert (one.J != J).all() and one.counts == dict(frames=T + 21, since=21, learned=T - n - 2 + 21 - n - 2)
    # the first command after a restart sees no history: c = theta[0] x
    fresh = pc.PredictorBank(n, 1.6, 0.99, 1e4, 20)
    fresh.push(x)
    fresh.restart()
    c0 = fresh.push(X[T:T + 1])
    assert np.array_equal(c0[0], (fresh.theta[:, 0] * X[T]).astype(np.float32))
    # frozen: theta and P stay, bit for bit; c, J, J0 go on
    th, P, J, J0 = [a.copy() for a in _state(fresh)]
    fresh.learning = False
    c = fresh.push(X[T + 1:T + 60])
    assert fresh.theta.tobytes() == th.tobytes() and fresh.P.tobytes() == P.tobytes()
    assert (fresh.J != J).all() and (fresh.J0 != J0).all() and np.abs(c).max() > 0      # (forget < 1: either way)
    assert fresh.counts["learned"] == T - n - 2
    fresh.learning = True
    fresh.push(X[T + 60:T + 61])
    assert (fresh.theta != th).any()


@pytest.mark.parametrize("delay", (0.0, 1.0, 1.5, 2.0))
def test_it_predicts(delay):
    """On the predictable series the predictor's sum of eps^2 over frames >= 500 is below 0.9 of what the best stable
    integrator gain of gain_grid(0, 1.2, 25) leaves, series by series its own best (measured 0.72 / 0.68 / 0.50 / 0.58 at
    delays 0 / 1 / 1.5 / 2 when the law was written down); order 1 cannot: it has nothing to extrapolate from."""
    grid = mg.gain_grid(0.0, 1.2, 25)
    with np.errstate(over="ignore", invalid="ignore"):      # (the unstable candidates of the grid diverge)
        Ji = mg.loop_rejection(X, grid, delay, nskip=500)
    st = mg.stable(grid, delay)
    best = np.where(st, Ji, np.inf).min(axis=-1).sum()
    ratio = {}
    for order in (4, 1):
        bank = pc.PredictorBank(order, delay, 1.0, 1e4, 500)
        bank.push(X)
        ratio[order] = float(bank.J.sum() / best)
    print("delay %g: predictor / best integrator: order 4 %.3f, order 1 %.3f" % (delay, ratio[4], ratio[1]))
    assert ratio[4] < 0.9
    assert ratio[1] > ratio[4]


def test_constructor_refusals():
    for kw in (dict(order=0), dict(order=9), dict(forget=0.0), dict(forget=1.5), dict(p0=0.0), dict(p0=float("inf")),
               dict(delay=2.5), dict(nskip=-1)):
        a = dict(order=4, delay=1.0, forget=1.0, p0=1e4, nskip=0)
        a.update(kw)
        with pytest.raises(ValueError, match=list(kw)[0]):
            pc.PredictorBank(**a)
    b = pc.PredictorBank(2, 1.0)
    b.push(np.zeros((1, 3)))
    with pytest.raises(ValueError, match="series"):
        b.push(np.zeros((1, 4)))
    with pytest.raises(ValueError, match="symmetric"):
        b.set(P=np.array([[[1.0, 0.5], [0.4, 1.0]]] * 3))
    with pytest.raises(ValueError, match="symmetric"):
        b.set(P=np.array([[[1.0, 0.0], [0.0, -1.0]]] * 3))
    th, P = np.full((3, 2), 0.5), np.array([[[2.0, 0.5], [0.5, 1.0]]] * 3)
    b.set(th, P)
    assert np.array_equal(b.theta, th) and np.array_equal(b.P, P)


def test_host_check_builds_and_passes(tmp_path):
    """predictor_host_check.cpp under the address and undefined-behaviour sanitizers: every refusal of the desc and the
    set validators, the frame counters, and aomarl_predictor_fn.h's update -- the text the kernel compiles -- for orders
    1 .. 8 against a plain-loop restatement."""
    exe = str(tmp_path / "predictor_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(CSRC, "predictor_host_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "predictor_host_check: ok"


def test_fn_header_against_the_statement(tmp_path):
    """The same host program prints theta, P, J, J0 and c of a series it is handed: the header's update against the NumPy
    statement, orders 1 / 3 / 8, forget 1 and 0.98, to 1e-9 of each array's maximum (c to one float32 ulp)."""
    exe = str(tmp_path / "predictor_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(CSRC, "predictor_host_check.cpp")])
    x = X[:200, 0].astype(np.float32)
    for order in (1, 3, 8):
        for forget in (1.0, 0.98):
            out = subprocess.run([exe, "run", str(order), "1.6", repr(forget), "1e4", "20"] + [repr(float(v)) for v in x],
                                 capture_output=True, text=True, timeout=60)
            assert out.returncode == 0, out.stderr
            v = np.array([float(t) for t in out.stdout.split()])
            n = order
            theta, P, J, J0, c = v[:n], v[n:n + n * n].reshape(n, n), v[n + n * n], v[n + n * n + 1], v[n + n * n + 2:]
            ref = pc.PredictorBank(order, 1.6, forget, 1e4, 20)
            cr = ref.push(x[:, None])[:, 0]
            for got, want in ((theta, ref.theta[0]), (P, ref.P[0]), (J, ref.J[0]), (J0, ref.J0[0])):
                assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (order, forget)
            assert c.size == cr.size and (np.abs(c - cr) <= np.spacing(np.abs(cr))).all()
