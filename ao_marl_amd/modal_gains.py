"""Modal gain optimisation: one integrator gain per Btt mode, found on a bank of loop filters.

The reference's parameter class carries `modopti`, `nrec`, `gmin`, `gmax`, `ngain` (shesha/config/PCONTROLLER.py:78-88)
and rtc_init.py:485-513 hands them to `init_modalOpti` / `modalControlOptimization`, which live in the native library
that is not part of the reference tree.  What is here is the published method (Gendron & Lena 1994): from recorded
OPEN-loop modal measurements, minimise the variance of the measured residual of each mode over a grid of gains -- in
the time domain, on this simulator's exact loop.  With x[t] = -s2m . slopes of frame t with the mirrors flat, one mode
of the loop (frame t = next_part_two, then next_part_one; the delay line forms the voltage of frame t from the commands
do_control left at frames t-1, t-2, t-3) obeys

    e[t] = x[t] - (wa c[t-1] + wb c[t-2] + wc c[t-3])          history before frame 0: zero
    c[t] = c[t-1] + g e[t]
    E/X  = (1 - z^-1) / (1 + (g wa - 1) z^-1 + g wb z^-2 + g wc z^-3)

for a linear sensor that measures the mirror as commanded (s2m . D . Btt = I on the kept modes); (wa, wb, wc) are the
delay-line weights of aomarl_apply_control.  J[env][mode][j] = sum over t >= nskip of e[t]^2 for gain g_j; the optimum
is the grid argmin among the stable candidates, ties -- and so all-zero (filtered) series -- taking the lowest gain, a
non-finite J counting as +inf.  g = 0 is the open loop (e = x: the pole at 1 is cancelled, nothing grows): a legal
candidate.

`LoopBank` / `loop_rejection` are the float64 NumPy statement: they DEFINE the bank and are the CPU path.
`NativeLoopBank` (aomarl_modopti_*, csrc/aomarl_modopti.hip) is its restatement on the GPU.  The law the gains enter
is VecRlSupervisor.set_modal_gains: m[t] = m[t-1] + gain * mgain[m] * e[t] in Btt coordinates.

`OnlineLoopBank` / `NativeOnlineLoopBank` / `OnlineModalGains` are the same bank ON-LINE: fed in closed loop with the
pseudo-open-loop modes x[t] = e[t] + v2m . voltage[t], with a forgetting factor, applied every `period` frames.

    python -m ao_marl_amd.modal_gains <config> [--nrec --gmin --gmax --ngain --envs --out gains.npz]
    python -m ao_marl_amd.modal_gains <config> --online [--period 256 --horizon 2048 --beta 1]
"""
import ctypes as C

import numpy as np

from . import attachments
from . import libaomarl as la

__all__ = ["gain_grid", "delay_weights", "stable", "pole_radius", "argmin_gain", "LoopBank", "loop_rejection",
           "NativeLoopBank", "record_open_loop", "ModalGainOptimizer", "optimize_modal_gains", "OnlineLoopBank",
           "NativeOnlineLoopBank", "OnlineModalGains"]


def gain_grid(gmin=0.0, gmax=1.0, ngain=15):
    """The reference's three parameters (PCONTROLLER.py:82-88): ngain gains from gmin to gmax, both included."""
    ngain = int(ngain)
    if ngain < 1:
        raise ValueError("ngain = %d: at least one gain" % ngain)
    if not (np.isfinite(gmin) and np.isfinite(gmax)) or gmax < gmin:
        raise ValueError("gmin = %r, gmax = %r: finite, gmin <= gmax" % (gmin, gmax))
    return np.linspace(float(gmin), float(gmax), ngain)


def delay_weights(delay):
    """(wa, wb, wc) of aomarl_apply_control: voltage = wa com + wb com1 + wc com2."""
    d = float(delay)
    if not 0.0 <= d <= 2.0:
        raise ValueError("delay = %r: the delay line holds two frames (0 <= delay <= 2)" % (delay,))
    return (1.0 - d, d, 0.0) if d <= 1.0 else (0.0, 2.0 - d, d - 1.0)


def pole_radius(gains, delay):
    """Largest |root| of z^3 + (g wa - 1) z^2 + g wb z + g wc for every gain (numpy.roots)."""
    wa, wb, wc = delay_weights(delay)
    g = np.asarray(gains, dtype=np.float64).reshape(-1)
    out = np.empty(g.size)
    for i, gi in enumerate(g):
        out[i] = np.inf if not np.isfinite(gi) else np.abs(np.roots([1.0, gi * wa - 1.0, gi * wb, gi * wc])).max()
    return out.reshape(np.shape(gains))


def stable(gains, delay):
    """May each gain be returned as an optimum?  All poles strictly inside the unit circle; g = 0 (the open loop, its
    pole at 1 cancelled by the numerator) counts as stable.  Agrees with mo_stable of csrc/aomarl_modopti_host.h
    (Jury's criterion, exact on the marginal cases of the usual grids: delay 1 with g = 1, delay 0 with g = 2).  The
    roots numpy finds carry round-off, so a radius within 1e-9 of the circle counts as marginal, not stable."""
    g = np.asarray(gains, dtype=np.float64)
    return (pole_radius(g, delay) < 1.0 - 1e-9) | (g == 0.0)


def argmin_gain(J, gains, stable_mask):
    """Index of the smallest J along the last axis among the stable candidates: a non-finite J counts as +inf, ties
    take the lowest GAIN; -1 where no candidate is stable."""
    J = np.asarray(J, dtype=np.float64)
    g = np.asarray(gains, dtype=np.float64).reshape(-1)
    ok = np.asarray(stable_mask, dtype=bool).reshape(-1)
    if J.shape[-1] != g.size or ok.size != g.size:
        raise ValueError("J has %d candidates, gains %d, stable %d" % (J.shape[-1], g.size, ok.size))
    if not ok.any():
        return np.full(J.shape[:-1], -1, dtype=np.int32)
    order = np.argsort(g, kind="stable")
    order = order[ok[order]]                                   # stable candidates, by ascending gain
    Jo = np.where(np.isfinite(J[..., order]), J[..., order], np.inf)
    return order[np.argmin(Jo, axis=-1)].astype(np.int32)      # argmin: the first of equals


class LoopBank(object):
    """The float64 statement of the filter bank, fed chunk by chunk: accumulate(x [nframes, ...series]) any number of
    times, then J ([...series, ngain]).  gains: [ngain] for every series or [...series, ngain] (one grid per series)."""

    def __init__(self, gains, delay, nskip=0):
        self.gains = np.asarray(gains, dtype=np.float64)
        if self.gains.ndim < 1 or self.gains.shape[-1] < 1 or not np.isfinite(self.gains).all():
            raise ValueError("gains: at least one, all finite")
        self.w = delay_weights(delay)
        self.delay, self.nskip = float(delay), int(nskip)
        if self.nskip < 0:
            raise ValueError("nskip = %d must not be negative" % self.nskip)
        self.frames, self.c, self.J = 0, None, None

    def reset(self):
        self.frames, self.c, self.J = 0, None, None

    def accumulate(self, x):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim < 1:
            raise ValueError("x must be [nframes, ...series]")
        shape = x.shape[1:] + (self.gains.shape[-1],)
        if self.c is None:
            np.broadcast_to(self.gains, shape)                 # raises when a per-series grid does not fit
            self.c = [np.zeros(shape) for _ in range(3)]
            self.J = np.zeros(shape)
        elif self.J.shape != shape:
            raise ValueError("x has series %s, the bank %s" % (x.shape[1:], self.J.shape[:-1]))
        wa, wb, wc = self.w
        c0, c1, c2 = self.c
        for t in range(x.shape[0]):
            e = x[t][..., None] - (wa * c0 + wb * c1 + wc * c2)
            cn = c0 + self.gains * e
            if self.frames >= self.nskip:
                self.J = self.J + e * e
            c0, c1, c2 = cn, c0, c1
            self.frames += 1
        self.c = [c0, c1, c2]
        return self

    def result(self):
        """(J, argmin index, stable mask [ngain] or per series)."""
        st = stable(self.gains, self.delay)
        if self.gains.ndim == 1:
            return self.J, argmin_gain(self.J, self.gains, st), st
        return self.J, None, st


def loop_rejection(x, gains, delay, nskip=0):
    """J[..., j] = sum over t >= nskip of e[t]^2 of the loop with gain g_j run on the open-loop series x [T, ...]
    (float64; the definition of the bank)."""
    return LoopBank(gains, delay, nskip).accumulate(x).J


class NativeLoopBank(object):
    """aomarl_modopti_* for [nenv][nmodes] series and one grid of gains (float32 values; `gains` holds them as
    float64, what the statement has to be run with).  accumulate(x): a float32 device tensor [nframes][nenv][nmodes]."""

    def __init__(self, nenv, nmodes, gains, delay, nskip=0, device="cuda:0"):
        import torch
        self.lib = la.load()
        self.device = torch.device(device)
        g32 = np.ascontiguousarray(np.asarray(gains, dtype=np.float32).reshape(-1))
        self.gains = g32.astype(np.float64)
        self.nenv, self.nmodes, self.ngain = int(nenv), int(nmodes), int(g32.size)
        self.delay, self.nskip = float(np.float32(delay)), int(nskip)      # (the descriptor's, and the simulator's, float)
        d = la.ModoptiDesc()
        d.nenv, d.nmodes, d.ngain, d.nskip, d.delay = self.nenv, self.nmodes, self.ngain, self.nskip, self.delay
        d.gains = la.fptr(g32) if g32.size else None
        self.ptr = C.c_void_p()
        if not torch.cuda.is_available():
            raise la.AomarlError("NativeLoopBank needs a GPU (the NumPy statement is LoopBank)")
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_modopti_create(C.byref(d), C.byref(self.ptr)))

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.aomarl_modopti_destroy(self.ptr)
            self.ptr = None

    def reset(self):
        la.check(self.lib.aomarl_modopti_reset(self.ptr))

    def accumulate(self, x, nframes=None):
        if x.dim() != 3 or tuple(x.shape[1:]) != (self.nenv, self.nmodes) or str(x.dtype) != "torch.float32" or \
                not x.is_cuda or x.stride(2) != 1 or x.stride(1) != self.nmodes or \
                (x.shape[0] > 1 and x.stride(0) < self.nenv * self.nmodes):
            raise ValueError("x must be a float32 device tensor [nframes][%d][%d] of contiguous frames" %
                             (self.nenv, self.nmodes))
        n = x.shape[0] if nframes is None else int(nframes)
        if not 0 <= n <= x.shape[0]:
            raise ValueError("nframes = %d of %d" % (n, x.shape[0]))
        if n == 0:
            return self
        stride = x.stride(0) if x.shape[0] > 1 else self.nenv * self.nmodes
        la.check(self.lib.aomarl_modopti_accumulate(self.ptr, x.data_ptr(), n, int(stride), la.raw_stream(self.device)))
        return self

    def result(self):
        """(J [nenv][nmodes][ngain] float64, argmin [nenv][nmodes] int32, stable [ngain] bool, frames): NumPy."""
        import torch
        J = torch.empty(self.nenv, self.nmodes, self.ngain, dtype=torch.float64, device=self.device)
        arg = torch.empty(self.nenv, self.nmodes, dtype=torch.int32, device=self.device)
        st = np.zeros(self.ngain, dtype=np.int32)
        n = C.c_longlong(0)
        la.check(self.lib.aomarl_modopti_result(self.ptr, J.data_ptr(), arg.data_ptr(), la.iptr(st), C.byref(n),
                                                la.raw_stream(self.device)))
        return J.cpu().numpy(), arg.cpu().numpy(), st.astype(bool), int(n.value)


def _pool_rows(pool, nenv):
    if pool not in ("all", None):
        raise ValueError("pool = %r: 'all' or None" % (pool,))
    return 1 if pool == "all" else int(nenv)


class OnlineLoopBank(object):
    """The float64 statement of the ON-LINE optimiser: the bank fed one pseudo-open-loop frame at a time while the loop
    is closed, with a forgetting factor, and an apply every `period` frames.

    x[t] = e[t] + p[t], e[t] = -s2m . slopes[t], p[t] = v2m . voltage[t]: the voltage apply_control applied in the
    next_part_two of the frame whose next_part_one measured slopes[t] -- whatever produced it.  push(x [nenv][nmodes]):

        eps = x - (wa c0 + wb c1 + wc c2);  c <- (c0 + g eps, c0, c1)            for every candidate g
        if frames since restart >= nskip:  J = forget * J + eps * eps

    and every `period` frames (counted over all frames pushed), once at least one frame has entered J:

        Jp = J (pool=None)  or  the sum of J over the environments in ascending order (pool="all")
        j* = argmin_gain(Jp, gains, stable);  G <- G + beta * (gains[j*] - G);  mgain(gain) = float32(G / gain)

    G: [nmodes] (pooled) or [nenv][nmodes]; G0 gives its start (default zeros: the open loop).  restart() -- an episode
    reset -- zeroes c0..c2 and the since-restart counter and keeps J and G.  With forget = 1 and no apply, J is
    LoopBank's, bit for bit."""

    def __init__(self, gains, delay, nskip=50, period=256, forget=1.0, beta=1.0, pool="all", G0=None):
        self.gains = np.asarray(gains, dtype=np.float64).reshape(-1)
        if self.gains.size < 1 or not np.isfinite(self.gains).all():
            raise ValueError("gains: at least one, all finite")
        self.w = delay_weights(delay)
        self.delay, self.nskip, self.period = float(delay), int(nskip), int(period)
        self.forget, self.beta, self.pool = float(forget), float(beta), pool
        _pool_rows(pool, 1)
        if self.nskip < 0:
            raise ValueError("nskip = %d must not be negative" % self.nskip)
        if self.period < 1:
            raise ValueError("period = %d: at least one frame between applies" % self.period)
        if not 0.0 < self.forget <= 1.0:
            raise ValueError("forget = %r: in (0, 1]" % (forget,))
        if not 0.0 < self.beta <= 1.0:
            raise ValueError("beta = %r: in (0, 1]" % (beta,))
        self.stable = stable(self.gains, self.delay)
        if not self.stable.any():
            raise ValueError("gains: no candidate is stable at delay %g (%s)" % (self.delay, self.gains))
        self.G = None if G0 is None else np.array(G0, dtype=np.float64)
        self.c = self.J = self.index = None
        self.frames = self.since = self.counted = self.updates = 0

    def restart(self):
        if self.c is not None:
            self.c = [np.zeros_like(self.J) for _ in range(3)]
        self.since = 0

    def push(self, x):
        """One frame x [nenv][nmodes]; True when this frame's apply changed G."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("x must be [nenv][nmodes], got shape %s" % (x.shape,))
        shape = x.shape + (self.gains.size,)
        if self.J is None:
            self.c = [np.zeros(shape) for _ in range(3)]
            self.J = np.zeros(shape)
            gshape = x.shape[1:] if self.pool == "all" else x.shape
            if self.G is None:
                self.G = np.zeros(gshape)
            elif self.G.shape != gshape:
                raise ValueError("G0 has shape %s, pool = %r needs %s" % (self.G.shape, self.pool, gshape))
        elif self.J.shape != shape:
            raise ValueError("x is %s, the bank %s" % (x.shape, self.J.shape[:-1]))
        wa, wb, wc = self.w
        c0, c1, c2 = self.c
        e = x[..., None] - (wa * c0 + wb * c1 + wc * c2)
        self.c = [c0 + self.gains * e, c0, c1]
        if self.since >= self.nskip:
            self.J = self.forget * self.J + e * e
            self.counted += 1
        self.frames += 1
        self.since += 1
        if self.frames % self.period == 0 and self.counted > 0:
            self.apply()
            return True
        return False

    def pooled(self):
        """What the argmin sees: J, or its sum over the environments in ascending order."""
        if self.pool != "all":
            return self.J
        Jp = self.J[0]
        for e in range(1, self.J.shape[0]):
            Jp = Jp + self.J[e]
        return Jp

    def apply(self):
        self.index = argmin_gain(self.pooled(), self.gains, self.stable)
        self.G = self.G + self.beta * (self.gains[self.index] - self.G)
        self.updates += 1
        return self.G

    def mgain(self, gain):
        """float32(G / gain): the factors on the scalar gain (a float32 on the device) that the apply writes"""
        return (self.G / np.float64(np.float32(gain))).astype(np.float32)


class NativeOnlineLoopBank(object):
    """aomarl_modopti_online_* (csrc/aomarl_modopti.hip): OnlineLoopBank on the GPU, fed through push(x) -- a float32
    device tensor [nenv][nmodes] -- or, attached to a simulator's context, by aomarl_do_control itself.  `gains` holds the
    float32 candidates as float64, `delay` the float32 delay: what the statement has to be run with."""

    def __init__(self, nenv, nmodes, gains, delay, nskip=50, period=256, forget=1.0, beta=1.0, pool="all", G0=None,
                 chunk=32, device="cuda:0"):
        import torch
        self.lib = la.load()
        self.device = torch.device(device)
        g32 = np.ascontiguousarray(np.asarray(gains, dtype=np.float32).reshape(-1))
        self.gains = g32.astype(np.float64)
        self.nenv, self.nmodes, self.ngain = int(nenv), int(nmodes), int(g32.size)
        self.rows = _pool_rows(pool, self.nenv)
        self.pool, self.delay = pool, float(np.float32(delay))
        self.sim = None
        d = la.ModoptiOnlineDesc()
        d.nenv, d.nmodes, d.ngain, d.nskip = self.nenv, self.nmodes, self.ngain, int(nskip)
        d.chunk, d.period, d.pool, d.delay = int(chunk), int(period), 1 if pool == "all" else 0, self.delay
        d.forget, d.beta = float(forget), float(beta)
        d.gains = la.fptr(g32) if g32.size else None
        g0 = None
        if G0 is not None:
            g0 = np.ascontiguousarray(G0, dtype=np.float64)
            if g0.size != self.rows * self.nmodes:
                raise ValueError("G0 has %d entries, pool = %r needs [%d][%d]" % (g0.size, pool, self.rows, self.nmodes))
            d.G0 = g0.ctypes.data_as(C.POINTER(C.c_double))
        self.ptr = C.c_void_p()
        if not torch.cuda.is_available():
            raise la.AomarlError("NativeOnlineLoopBank needs a GPU (the NumPy statement is OnlineLoopBank)")
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_modopti_online_create(C.byref(d), C.byref(self.ptr)))

    def __del__(self):
        if getattr(self, "ptr", None):
            if self.sim is not None and getattr(self.sim, "ctx", None):      # (a destroyed context has let go of it)
                self.detach()
            self.lib.aomarl_modopti_online_destroy(self.ptr)
            self.ptr = None

    def attach(self, sim):
        la.check(self.lib.aomarl_modopti_online_attach(sim.ctx, C.byref(sim.st), self.ptr))
        self.sim = sim

    def detach(self):
        if self.sim is not None:
            la.check(self.lib.aomarl_modopti_online_attach(self.sim.ctx, C.byref(self.sim.st), None))
            self.sim = None

    def restart(self):
        la.check(self.lib.aomarl_modopti_online_restart(self.ptr, la.raw_stream(self.device)))

    def push(self, x):
        if tuple(x.shape) != (self.nenv, self.nmodes) or str(x.dtype) != "torch.float32" or not x.is_cuda or \
                not x.is_contiguous():
            raise ValueError("x must be a contiguous float32 device tensor [%d][%d]" % (self.nenv, self.nmodes))
        la.check(self.lib.aomarl_modopti_online_push(self.ptr, x.data_ptr(), la.raw_stream(self.device)))
        return self

    def last(self):
        """The row pushed last (float32 device tensor [nenv][nmodes])."""
        import torch
        x = torch.empty(self.nenv, self.nmodes, dtype=torch.float32, device=self.device)
        la.check(self.lib.aomarl_modopti_online_last(self.ptr, x.data_ptr(), la.raw_stream(self.device)))
        return x

    def result(self):
        """(J [nenv][nmodes][ngain], index [rows][nmodes] of the last apply (-1: none yet), G [rows][nmodes], stable
        [ngain], counts): NumPy; counts = dict(frames, since, counted, updates).  Rows waiting in the ring are consumed."""
        import torch
        J = torch.empty(self.nenv, self.nmodes, self.ngain, dtype=torch.float64, device=self.device)
        arg = torch.empty(self.rows, self.nmodes, dtype=torch.int32, device=self.device)
        G = torch.empty(self.rows, self.nmodes, dtype=torch.float64, device=self.device)
        st = np.zeros(self.ngain, dtype=np.int32)
        n = (C.c_longlong * 4)()
        la.check(self.lib.aomarl_modopti_online_result(self.ptr, J.data_ptr(), arg.data_ptr(), G.data_ptr(), la.iptr(st),
                                                       n, la.raw_stream(self.device)))
        counts = dict(frames=int(n[0]), since=int(n[1]), counted=int(n[2]), updates=int(n[3]))
        return J.cpu().numpy(), arg.cpu().numpy(), G.cpu().numpy(), st.astype(bool), counts


def _open_loop_supervisor(sup, who="record_open_loop"):
    """Refuses the supervisor states in which a frame's slopes are not the ones the call order just measured."""
    attachments.refuse(sup, who, attachments.OPEN_LOOP)
    return sup


class OnlineModalGains(object):
    """The integrator whose modal gains are re-optimised in closed loop: an on-line bank attached to a VecRlSupervisor.
    gains: candidate ABSOLUTE gains (default gain_grid(); sorted, rounded to float32).  horizon: frames of memory,
    forget = exp(-1 / horizon); None: 1 (no forgetting).  native: the device bank fed by do_control itself; False: the
    NumPy statement fed through observe() by the caller after every next_part_one (slow: two read-backs per frame).

        opt = OnlineModalGains(sup, period=256, horizon=2048).start()
        ... run the loop; sup.reset() restarts the filters, J and G carry over ...
        opt.G, opt.updates;  opt.stop()"""
    slot = "online_modal_gains"
    row = attachments.TABLE[slot]

    def __init__(self, sup, gains=None, nskip=50, period=256, horizon=None, beta=1.0, pool="all", native=True, chunk=32):
        self.sup = sup
        g = gain_grid() if gains is None else np.asarray(gains, dtype=np.float64).reshape(-1)
        self.gains = np.unique(g.astype(np.float32)).astype(np.float64)
        self.nskip, self.period, self.beta, self.pool = int(nskip), int(period), float(beta), pool
        self.native, self.chunk = bool(native), int(chunk)
        if horizon is not None and not float(horizon) > 0.0:
            raise ValueError("horizon = %r: a positive number of frames, or None" % (horizon,))
        self.forget = 1.0 if horizon is None else float(np.exp(-1.0 / float(horizon)))
        self.delay = float(np.float32(sup.s.delay))
        self.rows = _pool_rows(pool, sup.sim.nenv)
        self.bank = None

    def start(self):
        sup = self.sup
        if self.bank is not None:
            raise RuntimeError("OnlineModalGains.start: already started")
        attachments.check(sup, self.slot)
        g = sup.gain
        if not float(g) > 0.0:
            raise RuntimeError("OnlineModalGains.start: the supervisor's gain is %r: no factor on it gives G" % (g,))
        mgain = sup.modal_gains
        if mgain is None:
            sup.set_modal_gains(np.ones((self.rows, sup.nmodes), dtype=np.float32))
            mgain = sup.modal_gains
        if mgain.shape[0] != self.rows:
            raise RuntimeError("OnlineModalGains.start: the modal gains have %d row(s), pool = %r needs %d"
                               % (mgain.shape[0], self.pool, self.rows))
        sup.ensure_slopes2modes()
        G0 = np.float64(np.float32(g)) * mgain.astype(np.float64)
        G0 = G0[0] if self.pool == "all" else G0
        if self.native:
            self.bank = NativeOnlineLoopBank(sup.sim.nenv, sup.nmodes, self.gains, self.delay, self.nskip, self.period,
                                             self.forget, self.beta, self.pool, G0, chunk=self.chunk, device=sup.sim.device)
            self.bank.attach(sup.sim)
        else:
            self.bank = OnlineLoopBank(self.gains, self.delay, self.nskip, self.period, self.forget, self.beta, self.pool, G0)
        attachments.attach(sup, self.slot, self)        # (checked above: the bank exists before the slot holds it)
        return self

    def observe(self):
        """native=False only: after next_part_one, push x = slopes2modes() + volts2modes(voltage) of the frame into the
        statement and set the gains an apply produced."""
        if self.native:
            raise RuntimeError("OnlineModalGains.observe: the native optimiser is fed by do_control itself")
        sim = self.sup.sim
        x = sim.slopes2modes().double() + sim.volts2modes(sim.voltage).double()
        if self.bank.push(x.cpu().numpy()):
            self.sup.sim.set_modal_gains(self.bank.mgain(self.sup.gain).reshape(self.rows, -1))

    def restart(self):
        if self.bank is not None:
            self.bank.restart()

    def stop(self):
        if self.bank is None:
            return
        if self.native:
            self.bank.detach()
        attachments.detach(self.sup, self.slot, self)
        self._final = (self.G, self.J, self.updates)
        self.bank = None

    def _read(self, k):
        if self.bank is None:
            final = getattr(self, "_final", None)
            return None if final is None else final[k]
        if self.native:
            J, _, G, _, counts = self.bank.result()
            return ((G[0] if self.pool == "all" else G), J, counts["updates"])[k]
        return (self.bank.G, self.bank.J, self.bank.updates)[k]

    @property
    def G(self):
        """The absolute gains in force: [nmodes] (pooled) or [nenv][nmodes]."""
        return self._read(0)

    @property
    def J(self):
        return self._read(1)

    @property
    def updates(self):
        return self._read(2)


def record_open_loop(sup, nrec, bank=None, chunk=64):
    """`nrec` frames from a fresh reset with the mirrors flat and the integrator off; the residual modes
    x[t] = -s2m . slopes of every frame go into a [chunk][nenv][nmodes] device buffer that feeds `bank`
    (a NativeLoopBank, or a LoopBank through the host) every `chunk` frames.  bank=None: the whole series comes back as
    a float32 device tensor [nrec][nenv][nmodes].  The supervisor is reset again afterwards (same seeds); its gain and
    modal gains are not touched."""
    import torch
    _open_loop_supervisor(sup)
    sim = sup.sim
    nrec, chunk = int(nrec), max(1, int(chunk))
    sup.ensure_slopes2modes()
    sup.reset()
    if float(sim.com.abs().max()) != 0.0:
        raise RuntimeError("record_open_loop: the commands are not zero behind reset()")
    buf = torch.empty(chunk, sim.nenv, sup.nmodes, dtype=torch.float32, device=sim.device)
    keep = torch.empty(nrec, sim.nenv, sup.nmodes, dtype=torch.float32, device=sim.device) if bank is None else None
    fill = 0

    def flush(n):
        if keep is not None or n == 0:
            return
        if isinstance(bank, LoopBank):
            bank.accumulate(buf[:n].cpu().numpy())
        else:
            bank.accumulate(buf, nframes=n)              # (same stream as the copies: the buffer is reused in order)

    for t in range(nrec):
        sup.next_part_two(None, linear_control=True)         # the flat mirrors applied (the delay line stays zero)
        sup.next_part_one(do_control=False)
        x = sim.slopes2modes()
        (keep[t] if keep is not None else buf[fill]).copy_(x)
        fill += 1
        if fill == chunk:
            flush(fill)
            fill = 0
    flush(fill)
    torch.cuda.synchronize(sim.device)                       # the bank has read the buffer before it is released
    sup.reset()
    return keep


class ModalGainOptimizer(object):
    """Gendron & Lena's optimisation for a VecRlSupervisor.  gains: the candidate ABSOLUTE gains (default:
    gain_grid()); they are sorted and rounded to float32, what the native bank takes.  nskip: frames left out of J (the
    transient from the zero history).  native: the GPU bank (aomarl_modopti_*) or the NumPy statement."""

    def __init__(self, sup, gains=None, nskip=50, native=True):
        self.sup = sup
        g = gain_grid() if gains is None else np.asarray(gains, dtype=np.float64).reshape(-1)
        self.gains = np.unique(g.astype(np.float32)).astype(np.float64)
        self.nskip, self.native = int(nskip), bool(native)
        self.delay = float(np.float32(sup.s.delay))      # the delay line's weights are formed from a float
        self.J = self.G = self.stable = self.index = None
        self.frames, self.pool = 0, None

    def run(self, nrec=2048, pool="all"):
        """Record nrec open-loop frames, return (J [nenv][nmodes][ngain], G, stable [ngain]).  pool="all": the J of
        all environments summed before the argmin, G is [nmodes]; pool=None: G is [nenv][nmodes]."""
        if pool not in ("all", None):
            raise ValueError("pool = %r: 'all' or None" % (pool,))
        sup = self.sup
        if self.native:
            bank = NativeLoopBank(sup.sim.nenv, sup.nmodes, self.gains, self.delay, self.nskip, device=sup.sim.device)
        else:
            bank = LoopBank(self.gains, self.delay, self.nskip)
        record_open_loop(sup, nrec, bank)
        if self.native:
            J, arg, st, frames = bank.result()
        else:
            (J, arg, st), frames = bank.result(), bank.frames
        if pool == "all":
            arg = argmin_gain(J.sum(axis=0), self.gains, st)
        if (arg < 0).any():
            raise RuntimeError("ModalGainOptimizer: no candidate gain is stable at delay %g (gains %s)" %
                               (self.delay, self.gains))
        self.J, self.index, self.stable, self.frames, self.pool = J, arg, st, frames, pool
        self.G = self.gains[arg]
        return self.J, self.G, self.stable

    def apply(self):
        """set_modal_gains(G / sup.gain): the factors on the supervisor's scalar gain that make gain * mgain = G."""
        if self.G is None:
            raise RuntimeError("ModalGainOptimizer.apply: run() first")
        g = self.sup.gain
        if g is None:
            raise RuntimeError("ModalGainOptimizer.apply: the supervisor has per-environment gains (set_gain with a "
                               "vector); set one scalar gain first")
        if float(g) == 0.0:
            raise RuntimeError("ModalGainOptimizer.apply: the supervisor's gain is 0: no factor on it gives G")
        mgain = (self.G / float(g)).astype(np.float32)
        self.sup.set_modal_gains(mgain)
        return mgain


def optimize_modal_gains(sup, nrec=None, gains=None, nskip=50, pool="all", native=True, apply=True):
    """The controller's own parameters as defaults (nrec, gmin, gmax, ngain of p_controllers[0]; nrec is taken as it
    is, nothing here needs a power of two).  Returns the ModalGainOptimizer, run and -- `apply` -- applied."""
    s = sup.s
    if gains is None:
        gains = gain_grid(getattr(s, "gmin", 0.0), getattr(s, "gmax", 1.0), getattr(s, "ngain", 15))
    opt = ModalGainOptimizer(sup, gains, nskip=nskip, native=native)
    opt.run(int(getattr(s, "nrec", 2048) if nrec is None else nrec), pool=pool)
    if apply:
        opt.apply()
    return opt


def _episode_strehl(sup, nsteps):
    """Long-exposure Strehl per environment of `nsteps` integrator-only closed-loop frames from a fresh reset."""
    sup.reset()
    for _ in range(nsteps):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()
    return sup.get_strehl()[:, 1].cpu().numpy()


def main(argv=None):
    """python -m ao_marl_amd.modal_gains <parameter file | builtin name> [--nrec 2048] [--gmin 0] [--gmax 1]
    [--ngain 15] [--envs 16] [--steps 1000] [--nskip 50] [--out gains.npz]"""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("config")
    ap.add_argument("--nrec", type=int, default=None)
    ap.add_argument("--gmin", type=float, default=None)
    ap.add_argument("--gmax", type=float, default=None)
    ap.add_argument("--ngain", type=int, default=None)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--nskip", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--online", action="store_true", help="also run the on-line optimiser from the scalar gain")
    ap.add_argument("--period", type=int, default=256)
    ap.add_argument("--horizon", type=float, default=None)
    ap.add_argument("--beta", type=float, default=1.0)
    a = ap.parse_args(argv)
    from . import params
    from .env import VecRlSupervisor
    cfg = params.load_param_file(a.config) if a.config.endswith(".py") else a.config
    sup = VecRlSupervisor(cfg, None, a.envs, device=a.device)
    s = sup.s
    grid = gain_grid(s.gmin if a.gmin is None else a.gmin, s.gmax if a.gmax is None else a.gmax,
                     s.ngain if a.ngain is None else a.ngain)
    sr0 = _episode_strehl(sup, a.steps)
    sr2 = Gon = None
    if a.online:                          # from the scalar gain: one episode to converge in, one to be measured in
        on = OnlineModalGains(sup, grid, nskip=a.nskip, period=a.period, horizon=a.horizon, beta=a.beta).start()
        _episode_strehl(sup, a.steps)
        sr2 = _episode_strehl(sup, a.steps)
        Gon, nup = on.G, on.updates
        on.stop()
        sup.set_modal_gains(None)
    opt = optimize_modal_gains(sup, nrec=a.nrec, gains=grid, nskip=a.nskip)
    sr1 = _episode_strehl(sup, a.steps)
    print("scalar gain %.3f: SR LE %.4f (mean of %d environments)" % (sup.gain, float(sr0.mean()), a.envs))
    print("modal gains (min %.3f, median %.3f, max %.3f): SR LE %.4f" %
          (opt.G.min(), float(np.median(opt.G)), opt.G.max(), float(sr1.mean())))
    if a.online:
        print("on-line modal gains (min %.3f, median %.3f, max %.3f; %d applies, second episode): SR LE %.4f" %
              (Gon.min(), float(np.median(Gon)), Gon.max(), nup, float(sr2.mean())))
    if a.out:
        np.savez(a.out, gains=opt.gains, G=opt.G, J=opt.J, stable=opt.stable, mgain=opt.G / sup.gain,
                 sr_le_scalar=sr0, sr_le_modal=sr1, frames=opt.frames,
                 **(dict(G_online=Gon, sr_le_online=sr2) if a.online else {}))


if __name__ == "__main__":
    main()
