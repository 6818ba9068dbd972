"""Modal predictive control: one recursive-least-squares predictor per (environment, Btt mode) on pseudo-open-loop modes.

Every other controller of this package is an integrator; none of them predicts across the loop delay.  Upstream has no
predictive controller in the reference tree: this is the published method (recursive least squares on pseudo-open-loop
telemetry) stated on this simulator's own loop model (modal_gains: frame t = next_part_two, then next_part_one; the
delay line forms the voltage of frame t from the commands left at frames t-1, t-2, t-3).

One independent series per (environment, mode).  x[t]: the pseudo-open-loop (POL) mode of frame t, e[t] + v2m . voltage[t]
as do_control forms it in float32, promoted to double.  (wa, wb, wc) = delay_weights(delay), n = order (1..8),
h[s] = (x[s], x[s-1], ..., x[s-n+1]), zero before the last restart, f = frames since it:

    phi  = wa h[t-1] + wb h[t-2] + wc h[t-3]      what the delay line will have applied at t, as a function of theta
    eps  = x[t] - theta . phi                      a-priori residual: the loop's e[t] for a constant theta
    if f >= nskip:   J = forget J + eps^2 ;  J0 = forget J0 + x[t]^2
    if learning and f >= n + 2:                    every regressor is a measured value, not restart padding
        q = P phi ; den = forget + phi . q
        theta += q (eps / den)
        P = (P - q q^T / den) / forget             symmetric by construction
        tr = trace(P);  if tr > n p0:  P *= n p0 / tr      an unexcited series must not blow P up under forget < 1
    c[t] = theta . h[t]                            theta AFTER the update; rounded once to float32

from theta = (1, 0, ..., 0) (the command is the last POL mode) and P = p0 I.  A restart (episode reset) zeroes the history
and f; theta, P, J, J0 carry over.  With forget = 1 the trace never grows and theta is exactly the ridge solution
argmin sum (x - theta . phi)^2 + |theta - theta0|^2 / p0 over the learned frames.

`PredictorBank` is the float64 NumPy statement: it DEFINES the filter and is the CPU path.  `NativePredictorBank`
(aomarl_predictor_*, csrc/aomarl_predictor.hip) is its restatement on the GPU; attached to a simulator's context,
aomarl_do_control runs it and commands com[t] = m2v . c[t] (+ the agents' action on the action modes through
aomarl_rl_control_modes).  `ModalPredictor` attaches one to a VecRlSupervisor.

    python -m ao_marl_amd.predictive <config> [--order 4 --horizon H --frames 1000 --envs 16]
"""
import ctypes as C

import numpy as np

from . import attachments
from . import libaomarl as la
from .modal_gains import delay_weights, record_open_loop

__all__ = ["MAX_ORDER", "PredictorBank", "NativePredictorBank", "ModalPredictor", "warm_start"]

MAX_ORDER = 8


def _check(order, delay, forget, p0, nskip):
    order, nskip = int(order), int(nskip)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError("order = %d: 1..%d past values" % (order, MAX_ORDER))
    if nskip < 0:
        raise ValueError("nskip = %d must not be negative" % nskip)
    if not 0.0 < float(forget) <= 1.0:
        raise ValueError("forget = %r: in (0, 1]" % (forget,))
    if not (float(p0) > 0.0 and np.isfinite(p0)):
        raise ValueError("p0 = %r: positive and finite" % (p0,))
    delay_weights(delay)
    return order, nskip


class PredictorBank(object):
    """The float64 statement of the predictor bank.  push(x [T, ...series]) -> c [T, ...series] float32; restart();
    theta [...series, n], P [...series, n, n], J, J0 [...series]; `learning` (False: theta and P frozen, c and J go on);
    frames / since / learned: frames pushed, since the last restart, frames that updated theta."""

    def __init__(self, order, delay, forget=1.0, p0=1e4, nskip=50):
        self.order, self.nskip = _check(order, delay, forget, p0, nskip)
        self.delay, self.forget, self.p0 = float(delay), float(forget), float(p0)
        self.w = delay_weights(delay)
        self.learning = True
        self.frames = self.since = self.learned = 0
        self._shape = self._th = self._P = self._xp = self._J = self._J0 = None

    def _init(self, shape):
        n, S = self.order, int(np.prod(shape, dtype=np.int64))
        self._shape = tuple(shape)
        self._th = np.zeros((S, n))
        self._th[:, 0] = 1.0
        self._P = np.broadcast_to(self.p0 * np.eye(n), (S, n, n)).copy()
        self._xp = np.zeros((S, n + 2))              # xp[:, k] = x[t-1-k]
        self._J, self._J0 = np.zeros(S), np.zeros(S)

    def restart(self):
        if self._xp is not None:
            self._xp = np.zeros_like(self._xp)
        self.since = 0

    def set(self, theta=None, P=None):
        """theta [...series, n], P [...series, n, n]: a checkpoint or a warm start (P symmetric, positive diagonal)."""
        for a, tail in ((theta, (self.order,)), (P, (self.order, self.order))):
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                if a.shape[a.ndim - len(tail):] != tail or not np.isfinite(a).all():
                    raise ValueError("set: expected [...series]%s finite values, got shape %s" % (list(tail), a.shape))
                if self._shape is None:
                    self._init(a.shape[:a.ndim - len(tail)])
        n = self.order
        if P is not None:
            P = np.asarray(P, dtype=np.float64).reshape(-1, n, n)
            if not np.array_equal(P, P.transpose(0, 2, 1)) or not (np.diagonal(P, axis1=1, axis2=2) > 0).all():
                raise ValueError("set: P must be symmetric with a positive diagonal")
            if P.shape != self._P.shape:
                raise ValueError("set: P has %d series, the bank %d" % (P.shape[0], self._P.shape[0]))
            self._P = P.copy()
        if theta is not None:
            theta = np.asarray(theta, dtype=np.float64).reshape(-1, n)
            if theta.shape != self._th.shape:
                raise ValueError("set: theta has %d series, the bank %d" % (theta.shape[0], self._th.shape[0]))
            self._th = theta.copy()

    def push(self, x):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim < 1:
            raise ValueError("x must be [nframes, ...series]")
        if self._shape is None:
            self._init(x.shape[1:])
        elif x.shape[1:] != self._shape:
            raise ValueError("x has series %s, the bank %s" % (x.shape[1:], self._shape))
        n, T = self.order, x.shape[0]
        wa, wb, wc = self.w
        xs = x.reshape(T, self._th.shape[0])
        c = np.empty(xs.shape, dtype=np.float32)
        th, P, xp, J, J0 = self._th, self._P, self._xp, self._J, self._J0
        cap = n * self.p0
        for t in range(T):
            xt = xs[t]
            phi = wa * xp[:, 0:n] + wb * xp[:, 1:n + 1] + wc * xp[:, 2:n + 2]
            eps = xt - (th * phi).sum(axis=1)
            if self.since >= self.nskip:
                J = self.forget * J + eps * eps
                J0 = self.forget * J0 + xt * xt
            if self.learning and self.since >= n + 2:
                q = (P * phi[:, None, :]).sum(axis=2)
                den = self.forget + (phi * q).sum(axis=1)
                th = th + q * (eps / den)[:, None]
                P = (P - q[:, :, None] * q[:, None, :] / den[:, None, None]) / self.forget
                tr = np.trace(P, axis1=1, axis2=2)
                over = tr > cap
                if over.any():
                    P[over] *= (cap / tr[over])[:, None, None]
                self.learned += 1
            h = np.concatenate([xt[:, None], xp[:, :n - 1]], axis=1)
            c[t] = (th * h).sum(axis=1)
            xp = np.concatenate([xt[:, None], xp[:, :-1]], axis=1)
            self.since += 1
            self.frames += 1
        self._th, self._P, self._xp, self._J, self._J0 = th, P, xp, J, J0
        return c.reshape(x.shape)

    def _get(self, a, tail):
        return None if a is None else a.reshape(self._shape + tail)

    @property
    def theta(self):
        return self._get(self._th, (self.order,))

    @property
    def P(self):
        return self._get(self._P, (self.order, self.order))

    @property
    def J(self):
        return self._get(self._J, ())

    @property
    def J0(self):
        return self._get(self._J0, ())

    @property
    def counts(self):
        return dict(frames=self.frames, since=self.since, learned=self.learned)


class NativePredictorBank(object):
    """aomarl_predictor_* (csrc/aomarl_predictor.hip): PredictorBank on the GPU for [nenv][nmodes] series, fed through
    push(x) -- a float32 device tensor [T][nenv][nmodes] -- or, attached to a simulator's context, by aomarl_do_control
    itself.  `delay` holds the float32 delay: what the statement has to be run with."""

    def __init__(self, nenv, nmodes, order, delay, forget=1.0, p0=1e4, nskip=50, device="cuda:0"):
        import torch
        self.lib = la.load()
        self.device = torch.device(device)
        self.nenv, self.nmodes, self.order, self.nskip = int(nenv), int(nmodes), int(order), int(nskip)
        self.delay, self.forget, self.p0 = float(np.float32(delay)), float(forget), float(p0)
        self.sim, self._learning = None, True
        d = la.PredictorDesc()
        d.nenv, d.nmodes, d.order, d.nskip = self.nenv, self.nmodes, self.order, self.nskip
        d.delay, d.forget, d.p0 = self.delay, self.forget, self.p0
        self.ptr = C.c_void_p()
        if not torch.cuda.is_available():
            raise la.AomarlError("NativePredictorBank needs a GPU (the NumPy statement is PredictorBank)")
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_predictor_create(C.byref(d), C.byref(self.ptr)))

    def __del__(self):
        if getattr(self, "ptr", None):
            if self.sim is not None and getattr(self.sim, "ctx", None):      # (a destroyed context has let go of it)
                self.detach()
            self.lib.aomarl_predictor_destroy(self.ptr)
            self.ptr = None

    def attach(self, sim):
        la.check(self.lib.aomarl_predictor_attach(sim.ctx, C.byref(sim.st), self.ptr))
        self.sim = sim

    def detach(self):
        if self.sim is not None:
            la.check(self.lib.aomarl_predictor_attach(self.sim.ctx, C.byref(self.sim.st), None))
            self.sim = None

    def restart(self):
        la.check(self.lib.aomarl_predictor_restart(self.ptr, la.raw_stream(self.device)))

    @property
    def learning(self):
        return self._learning

    @learning.setter
    def learning(self, on):
        la.check(self.lib.aomarl_predictor_set_learning(self.ptr, 1 if on else 0))
        self._learning = bool(on)

    def push(self, x, want_c=True):
        """x: float32 device tensor [T][nenv][nmodes] of contiguous frames; one launch.  Returns c (the same shape) or None."""
        import torch
        if x.dim() != 3 or tuple(x.shape[1:]) != (self.nenv, self.nmodes) or str(x.dtype) != "torch.float32" or \
                not x.is_cuda or x.stride(2) != 1 or x.stride(1) != self.nmodes or \
                (x.shape[0] > 1 and x.stride(0) < self.nenv * self.nmodes):
            raise ValueError("x must be a float32 device tensor [nframes][%d][%d] of contiguous frames" %
                             (self.nenv, self.nmodes))
        T = int(x.shape[0])
        c = torch.empty(T, self.nenv, self.nmodes, dtype=torch.float32, device=self.device) if want_c else None
        if T == 0:
            return c
        stride = x.stride(0) if T > 1 else self.nenv * self.nmodes
        la.check(self.lib.aomarl_predictor_push(self.ptr, x.data_ptr(), T, int(stride), c.data_ptr() if want_c else None,
                                                la.raw_stream(self.device)))
        return c

    def get(self):
        """(theta [nenv][nmodes][n], P [nenv][nmodes][n][n], J, J0 [nenv][nmodes], counts): NumPy float64."""
        import torch
        n, kw = self.order, dict(dtype=torch.float64, device=self.device)
        th = torch.empty(self.nenv, self.nmodes, n, **kw)
        P = torch.empty(self.nenv, self.nmodes, n, n, **kw)
        J, J0 = torch.empty(self.nenv, self.nmodes, **kw), torch.empty(self.nenv, self.nmodes, **kw)
        k = (C.c_longlong * 3)()
        la.check(self.lib.aomarl_predictor_get(self.ptr, th.data_ptr(), P.data_ptr(), J.data_ptr(), J0.data_ptr(), k,
                                               la.raw_stream(self.device)))
        counts = dict(frames=int(k[0]), since=int(k[1]), learned=int(k[2]))
        return th.cpu().numpy(), P.cpu().numpy(), J.cpu().numpy(), J0.cpu().numpy(), counts

    def set(self, theta=None, P=None):
        n, ns = self.order, self.nenv * self.nmodes
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        Pm = None if P is None else np.ascontiguousarray(P, dtype=np.float64)
        if th is not None and th.size != ns * n:
            raise ValueError("set: theta has %d entries, [%d][%d][%d] expected" % (th.size, self.nenv, self.nmodes, n))
        if Pm is not None and Pm.size != ns * n * n:
            raise ValueError("set: P has %d entries, [%d][%d][%d][%d] expected" % (Pm.size, self.nenv, self.nmodes, n, n))
        dp = C.POINTER(C.c_double)
        la.check(self.lib.aomarl_predictor_set(self.ptr, None if th is None else th.ctypes.data_as(dp),
                                               None if Pm is None else Pm.ctypes.data_as(dp)))

    def last(self):
        """(x, c): the row consumed last and the command modes it gave (float32 device tensors [nenv][nmodes])."""
        import torch
        x = torch.empty(self.nenv, self.nmodes, dtype=torch.float32, device=self.device)
        c = torch.empty_like(x)
        la.check(self.lib.aomarl_predictor_last(self.ptr, x.data_ptr(), c.data_ptr(), la.raw_stream(self.device)))
        return x, c

    theta = property(lambda self: self.get()[0])
    P = property(lambda self: self.get()[1])
    J = property(lambda self: self.get()[2])
    J0 = property(lambda self: self.get()[3])
    counts = property(lambda self: self.get()[4])


class ModalPredictor(object):
    """The predictive controller of a VecRlSupervisor: a predictor bank attached to its simulator.  order: past POL values
    per mode; horizon: frames of memory, forget = exp(-1 / horizon); None: 1 (no forgetting); p0: the start of P, in
    units of 1 / x^2.  native: the device bank run by do_control itself; False: the NumPy statement fed through observe()
    by the caller after every next_part_one (slow: read-backs per frame; linear_control=True only).

        pred = ModalPredictor(sup, order=4).start()
        pred.warm_start(2048); pred.freeze()      # optional: a trained, frozen filter
        ... run the loop; sup.reset() restarts the history, theta and P carry over ...
        pred.theta, pred.rejection;  pred.stop()"""
    slot = "modal_predictor"
    row = attachments.TABLE[slot]

    def __init__(self, sup, order=4, horizon=None, p0=1e4, nskip=50, native=True):
        self.sup = sup
        if horizon is not None and not float(horizon) > 0.0:
            raise ValueError("horizon = %r: a positive number of frames, or None" % (horizon,))
        self.forget = 1.0 if horizon is None else float(np.exp(-1.0 / float(horizon)))
        self.delay = float(np.float32(sup.s.delay))
        self.order, self.nskip = _check(order, self.delay, self.forget, p0, nskip)
        self.p0, self.native = float(p0), bool(native)
        self.bank, self._set_gains, self._final = None, False, None

    def _new_bank(self):
        sup = self.sup
        if self.native:
            return NativePredictorBank(sup.sim.nenv, sup.nmodes, self.order, self.delay, self.forget, self.p0, self.nskip,
                                       device=sup.sim.device)
        return PredictorBank(self.order, self.delay, self.forget, self.p0, self.nskip)

    def start(self):
        sup = self.sup
        if self.bank is not None:
            raise RuntimeError("ModalPredictor.start: already started")
        attachments.check(sup, self.slot)
        if float(sup.gain) == 0.0:
            raise RuntimeError("ModalPredictor.start: the supervisor's gain is 0: a do_control with gain 0 computes err "
                               "alone and is not a frame of the loop")
        if sup.modal_gains is None:                 # they route every step to the general chain; their values are not used
            sup.set_modal_gains(np.ones((1, sup.nmodes), dtype=np.float32))
            self._set_gains = True
        sup.ensure_slopes2modes()
        bank = self._new_bank()
        if self.native:
            bank.attach(sup.sim)
        else:
            bank.push(np.zeros((0, sup.sim.nenv, sup.nmodes)))       # (shapes the statement)
        self.bank = bank
        attachments.attach(sup, self.slot, self)        # (checked above: the bank exists before the slot holds it)
        return self

    def observe(self):
        """native=False only: after next_part_one, push x = slopes2modes() + volts2modes(voltage) of the frame into the
        statement and overwrite the command with m2v . c."""
        import torch
        if self.native:
            raise RuntimeError("ModalPredictor.observe: the native predictor is run by do_control itself")
        sup, sim = self.sup, self.sup.sim
        if getattr(sup, "last_modes", None) is not None:
            raise RuntimeError("ModalPredictor.observe: native=False serves the call-by-call order with "
                               "linear_control=True only (the agents' action would be composed on the integrator's modes)")
        x = sim.slopes2modes().double() + sim.volts2modes(sim.voltage).double()
        c = self.bank.push(x.float().cpu().numpy()[None])[0]
        com = c.astype(np.float64) @ np.asarray(sup.modes2volts, dtype=np.float64).T
        sim.set_com(torch.as_tensor(com.astype(np.float32), device=sim.device))

    def restart(self):
        if self.bank is not None:
            self.bank.restart()

    def freeze(self, on=True):
        """theta and P stop (on) or resume learning; c, J and J0 go on either way."""
        self.bank.learning = not on
        return self

    def warm_start(self, nrec):
        """`nrec` open-loop frames (record_open_loop: the mirrors flat, so the residual modes ARE the POL modes) pushed
        through the bank in one call, so that an episode can begin with a trained filter.  The supervisor is reset
        afterwards; the history starts over, theta and P are kept."""
        if self.bank is None:
            raise RuntimeError("ModalPredictor.warm_start: start() first")
        sup = self.sup
        if self.native:
            self.bank.detach()                      # (push is refused while do_control feeds it)
        try:
            x = record_open_loop(sup, nrec)
            self.bank.restart()
            if self.native:
                self.bank.push(x, want_c=False)
            else:
                self.bank.push(x.cpu().numpy())
            self.bank.restart()
        finally:
            if self.native:
                self.bank.attach(sup.sim)
        self.pol_rms = float(x.double().pow(2).mean().sqrt())
        return self

    def stop(self):
        if self.bank is None:
            return
        self._final = (self.theta, self.P, self.J, self.J0)
        if self.native:
            self.bank.detach()
        attachments.detach(self.sup, self.slot, self)
        if self._set_gains:
            self.sup.set_modal_gains(None)
            self._set_gains = False
        self.bank = None

    def _read(self, k):
        if self.bank is None:
            return None if self._final is None else self._final[k]
        if self.native:
            return self.bank.get()[k]
        return (self.bank.theta, self.bank.P, self.bank.J, self.bank.J0)[k]

    theta = property(lambda self: self._read(0))
    P = property(lambda self: self._read(1))
    J = property(lambda self: self._read(2))
    J0 = property(lambda self: self._read(3))

    @property
    def rejection(self):
        """J / J0 per (environment, mode): the residual the predictor's loop leaves over the open loop's (nan before a
        frame has been counted)."""
        J, J0 = self.J, self.J0
        with np.errstate(divide="ignore", invalid="ignore"):
            return J / J0

    def save(self, path):
        np.savez(path, theta=self.theta, P=self.P, order=self.order, delay=self.delay, forget=self.forget, p0=self.p0,
                 nskip=self.nskip, nenv=self.sup.sim.nenv, nmodes=self.sup.nmodes)

    def load(self, path):
        """theta and P of a checkpoint written by save() with the same order, delay and sizes."""
        if self.bank is None:
            raise RuntimeError("ModalPredictor.load: start() first")
        with np.load(path) as z:
            for k, mine in (("order", self.order), ("nenv", self.sup.sim.nenv), ("nmodes", self.sup.nmodes)):
                if int(z[k]) != mine:
                    raise ValueError("ModalPredictor.load: %s = %d in %s, %d here" % (k, int(z[k]), path, mine))
            if float(z["delay"]) != self.delay:
                raise ValueError("ModalPredictor.load: delay = %g in %s, %g here" % (float(z["delay"]), path, self.delay))
            self.bank.set(z["theta"], z["P"])
        return self


def warm_start(sup, nrec):
    """ModalPredictor.warm_start of the predictor attached to `sup`."""
    pred = getattr(sup, "modal_predictor", None)
    if pred is None:
        raise RuntimeError("warm_start: no predictor is attached to this supervisor (ModalPredictor(sup).start())")
    return pred.warm_start(nrec)


def _episode(sup, nsteps, nskip, observe=None):
    """`nsteps` closed-loop frames from a fresh reset without agents: (long-exposure Strehl per environment, the variance
    of the residual modes over frames >= nskip summed over the modes, mean of the environments)."""
    import torch
    sup.reset()
    acc = torch.zeros(sup.sim.nenv, sup.nmodes, dtype=torch.float64, device=sup.sim.device)
    for t in range(nsteps):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()
        if observe is not None:
            observe()
        if t >= nskip:
            acc += sup.sim.slopes2modes().double() ** 2
    var = float((acc / max(1, nsteps - nskip)).sum(dim=1).mean())
    return sup.get_strehl()[:, 1].cpu().numpy(), var


def main(argv=None):
    """python -m ao_marl_amd.predictive <parameter file | builtin name> [--order 4] [--horizon H] [--frames 1000]
    [--envs 16] [--p0 1e4] [--nrec 2048] [--nskip 50]"""
    import argparse
    from . import params
    from .env import VecRlSupervisor
    from .modal_gains import optimize_modal_gains
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("config")
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--horizon", type=float, default=None)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--p0", type=float, default=1e4)
    ap.add_argument("--nrec", type=int, default=2048)
    ap.add_argument("--nskip", type=int, default=50)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    cfg = params.load_param_file(a.config) if a.config.endswith(".py") else a.config
    sup = VecRlSupervisor(cfg, None, a.envs, device=a.device)
    sup.ensure_slopes2modes()
    rows = []
    sr, var = _episode(sup, a.frames, a.nskip)
    rows.append(("scalar integrator, gain %.3f" % sup.gain, sr, var))
    opt = optimize_modal_gains(sup, nrec=a.nrec, nskip=a.nskip)
    sr, var = _episode(sup, a.frames, a.nskip)
    rows.append(("modal integrator, off-line gains %.3f .. %.3f" % (opt.G.min(), opt.G.max()), sr, var))
    sup.set_modal_gains(None)
    kw = dict(order=a.order, horizon=a.horizon, p0=a.p0, nskip=a.nskip)
    pred = ModalPredictor(sup, **kw).start()
    sr, var = _episode(sup, a.frames, a.nskip)
    rows.append(("predictor, order %d, learning from the default start" % a.order, sr, var))
    pred.stop()
    pred = ModalPredictor(sup, **kw).start()
    pred.warm_start(a.nrec).freeze()
    sr, var = _episode(sup, a.frames, a.nskip)
    rows.append(("predictor, order %d, frozen after a warm start of %d frames" % (a.order, a.nrec), sr, var))
    rej = pred.rejection
    pred.stop()
    print("POL modes: rms %.4g over %d open-loop frames; p0 = %g, so p0 x rms^2 = %.4g" %
          (pred.pol_rms, a.nrec, a.p0, a.p0 * pred.pol_rms ** 2))
    for name, sr, var in rows:
        print("%-62s SR LE %.4f   sum of residual modal variances %.5g" % (name, float(sr.mean()), var))
    print("frozen predictor: J / J0 median %.4g, max %.4g over %d series" %
          (float(np.nanmedian(rej)), float(np.nanmax(rej)), rej.size))


if __name__ == "__main__":
    main()
