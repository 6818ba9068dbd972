"""Science field: Strehl and long-exposure PSF window in any number of directions per environment.

The loop's own science path looks in ONE direction, p_targets[0], through whole-pixel layer offsets.  A ScienceField looks at
the same state in T directions at once: each direction is traced bilinearly through the layers (natural stars: no cone)
and through the mirrors, and gets its own short- and long-exposure PSF window, phase variance and Strehl record.

Layers:
  field_offsets        directions (x", y") relative to the target -> float32 layer offsets [T][nlayers][2] on the pupil
                       (pupdiam) grid, every refusal by name
  field_trace_model    the atmosphere's phase [T][pupdiam][pupdiam], bilinear by the trace's rule (NumPy)
  FieldModel           per plane: amplitude, the W x W window of |DFT_npsf|^2 around zero frequency (W = 2 strehl_halfwin),
                       phase variance over the lit pixels, the record of 8 floats, the long-exposure sum; float64 NumPy:
                       the statement csrc/aomarl_field.hip is checked against, and the CPU path
  NativeField          aomarl_field_* (csrc/aomarl_field.hip)
  ScienceField         the public object, over a VecRlSupervisor or a simulator; it only reads the state, so it is no
                       row of attachments.TABLE and works beside any attachment

The record of a direction (the slots of aomarl_state.strehl):
  0 SE Strehl = window maximum / ref_peak    1 LE Strehl    2 phase variance    3 sum of the phase variances    4 frames
  5 peak on the window's edge    6 SE Strehl, fitted    7 LE Strehl, fitted
The fit is Target.comp_strehl(do_fit=True)'s: the peak fitted by two 1-D sincs through the maximum and its two neighbours
along x and along y, y(x) = A sinc(w (x - x0)); COMPASS's kernel is not in the reference tree, this is the restatement the
library uses everywhere (csrc/aomarl_kernels.hip: sinc_gain): Newton from the parabola through the three points, the
parabola's peak where the fit leaves 0 < w < 3, |x0| <= 0.6, 1 <= gain < 1.5, no fit for a maximum on the border.

Unpinned choices: a direction is measured RELATIVE to the target (direction (0, 0) is the target itself); one wavelength
per object (default: the target's); observe() looks at the state as it stands when it is called -- behind next_part_two
that is the frame's atmosphere under the command just applied, one delay step less than the loop's own record, which
looks at the frame's atmosphere under the previous command.

    python -m ao_marl_amd.field <config> [--radius arcsec] [--n N] [--stars x y gsalt ...] [--frames F]
"""
import ctypes as C
import os

import numpy as np

from . import geometry as G
from . import libaomarl as la
from .lgs import cone_trace_model

__all__ = ["field_offsets", "field_footprints", "field_trace_model", "sinc_gain", "fit_peak", "FieldModel", "NativeField",
           "ScienceField", "grid", "ring", "line", "MAX_DIRS_PER_LAUNCH"]

MAX_DIRS_PER_LAUNCH = 16                # AOMARL_FIELD_MAX_DIRS


# ------------------------------------------------------------------------------------------------ directions
def grid(radius, n):
    """n x n directions on a square grid over [-radius, radius]^2 arcsec, rows of constant y, x fastest"""
    t = np.linspace(-float(radius), float(radius), int(n)) if int(n) > 1 else np.zeros(1)
    return [(float(x), float(y)) for y in t for x in t]


def ring(n, radius):
    """n directions on a circle of `radius` arcsec, the first on the x axis"""
    a = 2 * np.pi * np.arange(int(n)) / int(n)
    return [(float(round(radius * np.cos(t), 9)), float(round(radius * np.sin(t), 9))) for t in a]


def line(radius, n):
    """n directions along the x axis from the target (0) out to `radius` arcsec"""
    return [(float(x), 0.0) for x in (np.linspace(0.0, float(radius), int(n)) if int(n) > 1 else np.zeros(1))]


def _as_directions(directions):
    try:
        d = np.array([[float(v) for v in p] for p in directions], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("field: directions are pairs (x arcsec, y arcsec)")
    if d.size == 0:
        raise ValueError("field: ndir = 0: at least one direction")
    if d.ndim != 2 or d.shape[1] != 2:
        raise ValueError("field: directions are pairs (x arcsec, y arcsec)")
    for k, p in enumerate(d):
        if not np.all(np.isfinite(p)):
            raise ValueError("field: direction %d: (%g, %g) is not finite" % (k, p[0], p[1]))
    return d


# ------------------------------------------------------------------------------------------------ offsets and trace
def field_footprints(sysm, off):
    """[T][nlayers][2][2]: the trace's coordinate (axis, corner) at the four corners of the pupil grid, as it is
    evaluated (float32 offsets)"""
    pd = int(sysm.geom.pupdiam)
    off = np.asarray(off, dtype=np.float32)
    corners = np.array([0.0, pd - 1.0])
    return corners[None, None, None, :] + off.astype(np.float64)[..., None]


def field_offsets(sysm, directions, itarget=0):
    """off [T][nlayers][2] float32 of the directions on the system `sysm` (geometry.build_system):
    off = float32(target atm_off_l + theta_d ARCSEC2RAD alt_l / pupixsize), theta_d relative to p_targets[itarget] (whose
    atm_off already holds pupdiff and the screen centring).  Each direction's footprint -- the trace's coordinate at the
    four corners of the pupil grid -- must lie inside every screen (the trace returns 0 outside one)."""
    d = _as_directions(directions)
    atm = sysm.atm
    alt = np.asarray(atm.alt, dtype=np.float64)
    base = np.asarray(sysm.targets[itarget].atm_off, dtype=np.float64).reshape(alt.size, 2)
    shift = d[:, None, :] * G.ARCSEC2RAD * alt[None, :, None] / float(atm.pupixsize)
    off = (base[None] + shift).astype(np.float32)
    fp = field_footprints(sysm, off)
    for k in range(d.shape[0]):
        for l in range(alt.size):
            dim = int(atm.dim_screens[l])
            for ax in range(2):
                for f in fp[k, l, ax]:
                    if not 0. <= f <= dim - 1:
                        raise ValueError(
                            "field: direction %d at (%g, %g) arcsec leaves screen %d (%d pixels, altitude %g m): its "
                            "footprint reaches %s = %.2f; the parameter file must declare a field of radius %g arcsec "
                            "(one more entry of p_targets or p_wfss at that radius)" % (
                                k, d[k, 0], d[k, 1], l, dim, alt[l], "xy"[ax], f, np.ceil(np.hypot(d[:, 0], d[:, 1]).max())))
    return off


def field_trace_model(screens, off, pupdiam, dtype=np.float64):
    """planes [T][pupdiam][pupdiam]: per direction the sum over the layers, in order, of screen l [dim][dim] sampled at
    (x, y) + off[d][l], bilinear by the trace's rule (zero outside a screen, the last line clamped) -- lgs.cone_trace_model
    without a cone (delta = 1).  float32: the arithmetic of the device's kernel."""
    ones = np.ones(len(screens))
    return np.stack([cone_trace_model(screens, [tuple(o) for o in off[k]], ones, int(pupdiam), dtype=dtype)
                     for k in range(len(off))])


# ------------------------------------------------------------------------------------------------ the sinc fit
def _sinc(t):
    return 1 - t * t / 6 if abs(t) < 1e-4 else np.sin(t) / t


def _dsinc(t):
    return -t / 3 if abs(t) < 1e-4 else (np.cos(t) - np.sin(t) / t) / t


def sinc_gain(ym, y0, yp, dtype=np.float64):
    """A / y(0) >= 1 of y(x) = A sinc(w (x - x0)) through (-1, ym), (0, y0), (1, yp) (module docstring); dtype: the
    arithmetic (np.float32: every operation in single precision)"""
    f = np.dtype(dtype).type
    ym, y0, yp, one = f(ym), f(y0), f(yp), f(1)
    if not y0 > 0:
        return 1.0
    rm, rp = ym / y0, yp / y0
    a, b = f(0.5) * (rm + rp) - one, f(0.5) * (rp - rm)
    if not a < f(-1e-6):
        return 1.0
    x0 = min(f(0.5), max(f(-0.5), -b / (f(2) * a)))
    gpar = one - b * b / (f(4) * a)
    w = np.sqrt(f(-6) * a / gpar)
    w = f(1e-3) if not w > f(1e-3) else min(w, f(3))
    for _ in range(8):
        f0, d0 = _sinc(w * x0), _dsinc(w * x0)
        fm, dm = _sinc(w * (one + x0)), _dsinc(w * (one + x0))
        fp, dp = _sinc(w * (one - x0)), _dsinc(w * (one - x0))
        F1, F2 = fm - rm * f0, fp - rp * f0
        J11, J12 = (one + x0) * dm - rm * x0 * d0, w * dm - rm * w * d0
        J21, J22 = (one - x0) * dp - rp * x0 * d0, -w * dp - rp * w * d0
        det = J11 * J22 - J12 * J21
        if not abs(det) > f(1e-12):
            break
        w = w - (F1 * J22 - F2 * J12) / det
        x0 = x0 - (J11 * F2 - J21 * F1) / det
        w = f(1e-3) if not w > f(1e-3) else min(w, f(3))
        x0 = min(f(0.6), max(f(-0.6), x0))
    g = one / _sinc(w * x0)
    if 1 <= g < 1.5:
        return float(g)
    return float(gpar) if 1 <= gpar < 1.5 else 1.0


def fit_peak(img, dtype=np.float64):
    """(maximum, fitted peak, on the edge) of a window: the first maximum in row-major order, its gain along x times its
    gain along y; a maximum on the border has no neighbours: no fit"""
    img = np.asarray(img, dtype=dtype)
    ny, nx = img.shape
    arg = int(np.argmax(img))
    ay, ax = divmod(arg, nx)
    m = float(img[ay, ax])
    if ax == 0 or ay == 0 or ax == nx - 1 or ay == ny - 1:
        return m, m, True
    gx = sinc_gain(img[ay, ax - 1], m, img[ay, ax + 1], dtype)
    gy = sinc_gain(img[ay - 1, ax], m, img[ay + 1, ax], dtype)
    f = np.dtype(dtype).type
    return m, float(f(m) * f(gx) * f(gy)), False


# ------------------------------------------------------------------------------------------------ the model
class FieldModel(object):
    """The PSF side on the system `s` (system.SimArrays: spupil, npsf, strehl_halfwin) at one wavelength `Lambda` microns
    (default: the target's).  dtype: np.float64 (the definition) or np.float32 (the same statement in single precision,
    the phase wrapped before the sine as the device wraps it: the yardstick of the device's error)."""

    def __init__(self, s, Lambda=None, dtype=np.float64):
        lam = float(s.tar_lambda if Lambda is None else Lambda)
        if not lam > 0 or not np.isfinite(lam):
            raise ValueError("field: Lambda = %r microns must be positive and finite" % (Lambda,))
        self.s, self.Lambda, self.dtype = s, lam, np.dtype(dtype)
        self.ctype = np.complex128 if self.dtype == np.float64 else np.complex64
        self.pd, self.npsf, self.hw = int(s.pupdiam), int(s.npsf), int(s.strehl_halfwin)
        self.W = 2 * self.hw
        self.pupil = np.asarray(s.spupil, dtype=np.float64).reshape(self.pd, self.pd)
        self.lit = self.pupil != 0
        self.ref_peak = float(np.sum(np.asarray(s.spupil, dtype=np.float32), dtype=np.float64))**2
        k = np.arange(-self.hw, self.hw)[:, None] * np.arange(self.pd)[None, :]
        self.E = np.exp(-2j * np.pi * (k % self.npsf) / self.npsf).astype(self.ctype)        # [W][pd]

    def amplitude(self, phase):
        """spupil exp(2 pi i phase / Lambda) [pd][pd], zero off the pupil"""
        dt = self.dtype.type
        ph = np.asarray(phase, dtype=self.dtype).reshape(self.pd, self.pd)
        t = ph * dt(1.0 / self.Lambda)
        if self.dtype == np.float32:
            t = (t - np.rint(t)).astype(np.float32)
        ang = (dt(2 * np.pi) * t).astype(self.dtype)
        a = (self.pupil.astype(self.dtype) * (np.cos(ang) + 1j * np.sin(ang))).astype(self.ctype)
        a[~self.lit] = 0
        return a

    def window(self, phase):
        """|DFT_npsf(amplitude)|^2 on the frequencies [-hw, hw)^2: [W][W], row ky, column kx"""
        g = (self.E @ self.amplitude(phase)) @ self.E.T
        return (g.real.astype(self.dtype)**2 + g.imag.astype(self.dtype)**2).astype(self.dtype)

    def variance(self, phase):
        """the phase variance over the lit pixels (float32: about the pivot at the grid's centre, as the device sums)"""
        ph = np.asarray(phase, dtype=self.dtype).reshape(self.pd, self.pd)
        if self.dtype == np.float64:
            return float(np.var(ph[self.lit]))
        d = (ph - ph[self.pd // 2, self.pd // 2])[self.lit].astype(np.float32)
        n = np.float32(d.size)
        mean = np.sum(d, dtype=np.float32) / n
        return float(np.sum(d * d, dtype=np.float32) / n - mean * mean)

    def new_state(self, *lead):
        """(record [..][8], le [..][W][W]) zeroed, float64"""
        return np.zeros(tuple(lead) + (8,)), np.zeros(tuple(lead) + (self.W, self.W))

    def commit(self, phase, record, le, window=None):
        """One observation of one plane into its record [8] and long-exposure sum [W][W] (in place); returns the window"""
        win = np.asarray(self.window(phase) if window is None else window, dtype=np.float64)
        var = self.variance(phase)
        le[:] = (le.astype(self.dtype) + win.astype(self.dtype)).astype(np.float64)          # (float32: the sum rounded too)
        cnt = record[4] + 1.0
        m, mfit, edge = fit_peak(win, self.dtype)
        ml, mlfit, _ = fit_peak(le, self.dtype)
        record[:] = (m / self.ref_peak, ml / cnt / self.ref_peak, var, record[3] + var, cnt, 1.0 if edge else 0.0,
                     mfit / self.ref_peak, mlfit / cnt / self.ref_peak)
        return win

    def observe(self, planes, record, le):
        """planes [T][pd][pd] into record [T][8] and le [T][W][W]; returns the windows [T][W][W]"""
        return np.stack([self.commit(planes[d], record[d], le[d]) for d in range(len(planes))])


# ------------------------------------------------------------------------------------------------ the device object
class _DeviceView(object):
    """a device buffer the library owns, as the array interface torch.as_tensor reads"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class NativeField(object):
    """aomarl_field_* (csrc/aomarl_field.hip) on a HipSim's context.  `record_view` [nenv][T][8] and `le_view`
    [nenv][T][W][W] are views of the buffers the object owns: they live as long as it does."""

    def __init__(self, sim, off, Lambda):
        import torch
        if not torch.cuda.is_available():
            raise la.AomarlError("NativeField needs a GPU (the NumPy statements are field_trace_model and FieldModel)")
        self.lib, self.sim, self.device = la.load(), sim, sim.device
        self.off = np.ascontiguousarray(off, dtype=np.float32)
        if self.off.ndim != 3 or self.off.shape[2] != 2:
            raise ValueError("off must be [T][nlayers][2]")
        self.T, self.nenv = int(self.off.shape[0]), int(sim.nenv)
        self.W, self.pd = 2 * int(sim.s.strehl_halfwin), int(sim.s.pupdiam)
        d = la.FieldDesc()
        d.ndir, d.nlayers, d.off, d.inv_lambda = self.T, int(self.off.shape[1]), la.fptr(self.off), 1.0 / float(Lambda)
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_field_create(sim.ctx, self.nenv, C.byref(d), C.byref(self.handle)))
            rec, le = C.c_void_p(), C.c_void_p()
            la.check(self.lib.aomarl_field_get(self.handle, 0, C.byref(rec), C.byref(le), self._stream()))
            self.record_view = torch.as_tensor(_DeviceView(rec.value, (self.nenv, self.T, 8)), device=self.device)
            self.le_view = torch.as_tensor(_DeviceView(le.value, (self.nenv, self.T, self.W, self.W)), device=self.device)

    def _stream(self):
        return la.raw_stream(self.device)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                import torch
                torch.cuda.synchronize(self.device)
                self.lib.aomarl_field_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _flags(self, atm, dms):
        return (la.TRACE_ATMOS if atm else 0) | (la.TRACE_DMS if dms else 0)

    def _shapes(self, dms):
        # shapes a deferred apply_control left to the frame kernel: formed here, the simulator's bookkeeping untouched
        # (the loop goes on evaluating them from the voltages, exactly as it would without an observer)
        sim = self.sim
        if dms and getattr(sim, "_stale", False):
            la.check(self.lib.aomarl_materialize_dm_shape(sim.ctx, C.byref(sim.st), 0, sim.nenv, self._stream()))

    def observe(self, atm=True, dms=True, env_begin=0, env_count=None):
        n = self.nenv - env_begin if env_count is None else int(env_count)
        self._shapes(dms)
        la.check(self.lib.aomarl_field_observe(self.handle, self.sim.ctx, C.byref(self.sim.st), int(env_begin), n,
                                               self._flags(atm, dms), self._stream()))

    def trace(self, planes, atm=True, dms=True, mask=False, reset=True, env_begin=0, env_count=None):
        n = self.nenv - env_begin if env_count is None else int(env_count)
        if tuple(planes.shape) != (self.nenv, self.T, self.pd, self.pd) or str(planes.dtype) != "torch.float32" or \
                not planes.is_cuda or not planes.is_contiguous():
            raise ValueError("planes must be a contiguous float32 device tensor [%d][%d][%d][%d]" % (
                self.nenv, self.T, self.pd, self.pd))
        self._shapes(dms)
        fl = self._flags(atm, dms) | (la.TRACE_RESET if reset else 0) | (la.TRACE_MASK if mask else 0)
        la.check(self.lib.aomarl_field_trace(self.handle, self.sim.ctx, C.byref(self.sim.st), planes.data_ptr(), int(env_begin),
                                             n, fl, self._stream()))
        return planes

    def reset(self, env_begin=0, env_count=None):
        n = self.nenv - env_begin if env_count is None else int(env_count)
        la.check(self.lib.aomarl_field_reset(self.handle, int(env_begin), n, self._stream()))

    def attach_mirrors(self, native_mcao, off, dm1):
        """the field sees the mirrors at altitude of `native_mcao` (mcao.NativeMcao) from now on: off [T][M][2], dm1 [T][M]"""
        v = native_mcao.view(off, dm1)
        la.check(self.lib.aomarl_field_attach_mirrors(self.handle, native_mcao.handle, C.byref(v[0])))
        self._mirrors = native_mcao                     # (kept alive: the field reads its planes)

    def detach_mirrors(self):
        la.check(self.lib.aomarl_field_detach_mirrors(self.handle))
        self._mirrors = None

    def fit(self):
        """the long exposure's fit into slot 7 of every record"""
        la.check(self.lib.aomarl_field_get(self.handle, 1, None, None, self._stream()))


# ------------------------------------------------------------------------------------------------ the public object
class ScienceField(object):
    """T science directions on a VecRlSupervisor (or on a simulator, with `sysm` = its geometry.build_system result).

        fld = ScienceField(sup, line(20, 5))           # arcsec, relative to the target
        ... sup.next_part_one(); sup.next_part_two(...); fld.observe() ...      # or fld.run(nframes)
        fld.strehl()                                    # [nenv][T][4]: SE, LE, phase variance, its mean (get_strehl's)

    observe() looks at the state as it stands (module docstring); it only reads the simulator.  On a CPU simulator with one
    oracle per environment (`sim.sims`) it runs FieldModel.  mirrors: a mcao.MultiConjugate whose mirrors at altitude every
    direction sees through its own footprint (behind the pupil mirrors); while one is attached to the supervisor, a field
    without it refuses to observe."""

    def __init__(self, sup_or_sim, directions, Lambda=None, sysm=None, mirrors=None):
        self.sup = sup_or_sim if hasattr(sup_or_sim, "sim") else None
        self.sim = self.sup.sim if self.sup is not None else sup_or_sim
        sysm = sysm if sysm is not None else getattr(sup_or_sim, "sysm", None)
        if sysm is None:
            raise ValueError("ScienceField: on a simulator, pass sysm (the geometry.build_system result it was built from)")
        self.s = s = self.sim.s
        self.directions = _as_directions(directions)
        self.T, self.nenv = int(self.directions.shape[0]), int(self.sim.nenv)
        for d in s.dms:
            if float(d.alt) != 0.:
                raise NotImplementedError("ScienceField: a mirror conjugated to %g m is seen differently from every "
                                          "direction; only mirrors in the pupil (alt = 0) are covered" % d.alt)
        self.Lambda = float(s.tar_lambda if Lambda is None else Lambda)
        if not self.Lambda > 0 or not np.isfinite(self.Lambda):
            raise ValueError("field: Lambda = %r microns must be positive and finite" % (Lambda,))
        self.off = field_offsets(sysm, self.directions)
        self.mirrors, self.mir_view = mirrors, None
        if mirrors is not None:
            from .mcao import mirror_offsets
            owner = mirrors.sup.sim if getattr(mirrors, "sup", None) is not None else getattr(mirrors, "sim", None)
            if owner is not self.sim:
                raise ValueError("ScienceField: mirrors is a MultiConjugate (or a NativeMcao) on another simulator")
            self.mir_view = mirror_offsets(sysm, mirrors.mirrors, self.directions, "pupil")
        self.device = str(self.sim.device)
        self.W, self.pd = 2 * int(s.strehl_halfwin), int(s.pupdiam)
        if self.device == "cpu":
            self.native = None
            self.model = FieldModel(s, self.Lambda)
            self._record, self._le = self.model.new_state(self.nenv, self.T)
        else:
            self.native = NativeField(self.sim, self.off, self.Lambda)
            self.model = None
            if mirrors is not None:
                self.native.attach_mirrors(mirrors.mc, *self.mir_view)

    # ---- what the CPU path needs
    def _oracles(self):
        sims = getattr(self.sim, "sims", None)
        if sims is None:
            raise NotImplementedError("the field's trace on the CPU needs a simulator with one oracle per environment "
                                      "(`sims`); field_trace_model is the NumPy statement")
        return sims

    def _cpu_planes(self, e, atm=True, dms=True):
        o = self._oracles()[e]
        pl = field_trace_model(o.screens, self.off, self.pd) if atm else np.zeros((self.T, self.pd, self.pd))
        if dms:
            keep = o.tar_phase.copy()                      # the oracle's own science phase is not ours to change
            o.raytrace_target(atm=False, dms=True, reset=True)
            pl = pl + np.asarray(o.tar_phase, dtype=np.float64)[None]
            o.tar_phase[:] = keep
            if self.mirrors is not None:
                from .mcao import mirrors_add_model
                pl = mirrors_add_model(pl, [np.asarray(sh[e], dtype=np.float64) for sh in self.mirrors.alt_shapes()],
                                       *self.mir_view)
        return pl

    def _range(self, env_begin, env_count):
        n = self.nenv - env_begin if env_count is None else int(env_count)
        if env_begin < 0 or n < 1 or env_begin + n > self.nenv:
            raise ValueError("ScienceField: environments %d .. +%d of %d" % (env_begin, n, self.nenv))
        return int(env_begin), n

    def _refuse_in_flight(self, who):
        sim = self.sim
        att = getattr(self.sup, "lgs", None)
        # (mirrors may be the attachment or the device object that owns its planes)
        if getattr(att, "altitude_mirrors", False) and self.mirrors is not att and \
                (self.mirrors is None or att.mc is None or getattr(self.mirrors, "mc", None) is not att.mc):
            raise RuntimeError("%s: a MultiConjugate is attached: every direction sees its mirrors at altitude through "
                               "its own footprint; build the field with mirrors=<the MultiConjugate> (or its field())" % who)
        if getattr(sim, "_twin", None) is not None and sim.frame_pipeline_state()[0]:
            raise RuntimeError("%s: a pipelined frame is in flight (the frames run a step ahead of the chains)" % who)
        pending = getattr(sim, "prefetch_reset_pending", None)
        if pending is not None and pending():
            raise RuntimeError("%s: a prefetched reset is in flight" % who)

    # ---- the interface
    def observe(self, env_begin=0, env_count=None):
        """Every direction of the environments of the range, of the state as it stands, into the records and the
        long-exposure sums.  On the device: one call, asynchronous, no read-back."""
        self._refuse_in_flight("ScienceField.observe")
        b, n = self._range(env_begin, env_count)
        if self.native is not None:
            self.native.observe(True, True, b, n)
            return
        sims = self._oracles()
        for e in range(b, b + n):
            self.model.observe(self._cpu_planes(e), self._record[e], self._le[e])

    def trace(self, atm=True, dms=True, env_begin=0, env_count=None):
        """The traced planes [nenv][T][pupdiam][pupdiam] in microns (rows outside the range are zero)"""
        self._refuse_in_flight("ScienceField.trace")
        b, n = self._range(env_begin, env_count)
        if self.native is not None:
            import torch
            pl = torch.zeros(self.nenv, self.T, self.pd, self.pd, dtype=torch.float32, device=self.sim.device)
            return self.native.trace(pl, atm, dms, False, True, b, n)
        sims = self._oracles()
        out = np.zeros((self.nenv, self.T, self.pd, self.pd))
        for e in range(b, b + n):
            out[e] = self._cpu_planes(e, atm, dms)
        return out

    def reset(self, env_begin=0, env_count=None):
        b, n = self._range(env_begin, env_count)
        if self.native is not None:
            self.native.reset(b, n)
        else:
            self._record[b:b + n], self._le[b:b + n] = 0., 0.

    @property
    def record(self):
        """[nenv][T][8] (module docstring), slot 7 fitted; a copy"""
        if self.native is not None:
            self.native.fit()
            return self.native.record_view.clone()
        return self._record.copy()

    def strehl(self, do_fit=True):
        """[nenv][T][4]: SE Strehl, LE Strehl, phase variance, mean phase variance -- get_strehl's tuple per direction"""
        r = self.record
        xp = np if self.native is None else __import__("torch")
        cnt = r[..., 4]
        avg = xp.where(cnt > 0, r[..., 3] / xp.maximum(cnt, xp.ones_like(cnt)), xp.zeros_like(cnt))
        i, j = (6, 7) if do_fit else (0, 1)
        return xp.stack([r[..., i], r[..., j], r[..., 2], avg], -1)

    def le_image(self):
        """[nenv][T][W][W]: the long-exposure window, divided by the frame count (zero before the first observe)"""
        if self.native is not None:
            import torch
            cnt = self.native.record_view[..., 4].clamp(min=1)
            return self.native.le_view / cnt[..., None, None]
        return self._le / np.maximum(self._record[..., 4], 1.0)[..., None, None]

    def run(self, nframes, action=None):
        """nframes of the supervisor's loop with an observe() behind every next_part_two (action None: the integrator)"""
        if self.sup is None:
            raise RuntimeError("ScienceField.run: built on a simulator; drive its loop and call observe()")
        sup = self.sup
        for _ in range(int(nframes)):
            sup.next_part_one()
            sup.next_part_two(action, linear_control=action is None)
            self.observe()
        return self.strehl()


# ------------------------------------------------------------------------------------------------ command line
def strehl_against_angle(sup, directions, nframes, mirrors=None):
    """long-exposure Strehl [T] (mean over the environments, fitted) of nframes of the loop as it is set up, behind a
    reset, and the loop's own on-axis figure.  mirrors: the attached mcao.MultiConjugate, if one is"""
    fld = ScienceField(sup, directions, mirrors=mirrors)
    sup.reset()
    st = fld.run(nframes)
    le = st[..., 1]
    le = le.mean(0).cpu().numpy() if hasattr(le, "cpu") else le.mean(0)
    return np.asarray(le, dtype=np.float64), float(sup.get_strehl()[:, 1].mean())


def print_tomography(sup, stars, dirs, nframes):
    """the rows of laser tomography on the same seeds: one calibration, the stars' mean (the ground-layer loop), then the
    MMSE reconstructor with the pseudo-open-loop term"""
    from .tomography import LaserTomography
    t = LaserTomography(sup, stars, reconstructor="mean", polc=False)
    t.calibrate()
    for rec in ("mean", "tomo"):
        t.set_reconstructor(rec, rec == "tomo")
        t.start()
        try:
            le, own = strehl_against_angle(sup, dirs, nframes)
        finally:
            t.stop()
        print("%-28s" % ("laser tomography, " + rec) + "".join("%8.4f" % v for v in le) + "   %8.4f" % own, flush=True)


def main(argv=None):
    import argparse
    from . import params as P
    from .env import VecRlSupervisor
    from .tomography import with_field
    from .tomography import ring as star_ring
    ap = argparse.ArgumentParser(prog="python -m ao_marl_amd.field",
                                 description="Long-exposure Strehl against the field angle on the same seeds: the NGS "
                                             "integrator and, with --stars, laser tomography with the stars' mean "
                                             "(ground layer) and with the MMSE reconstructor")
    ap.add_argument("config", nargs="?", default="production_sh_10x10_2m",
                    help="a built-in configuration or a parameter file (.py)")
    ap.add_argument("--radius", type=float, default=20., help="arcsec: the directions run from the target out to it")
    ap.add_argument("--n", type=int, default=5, help="directions along the line")
    ap.add_argument("--stars", type=float, nargs="*", default=None, metavar="V",
                    help="x y gsalt per star (no value: 4 stars at 90 km on a circle of --radius)")
    ap.add_argument("--field", type=float, default=None, help="the declared field radius in arcsec (default: radius + 5)")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--nfilt", type=int, default=5, help="Btt modes filtered from the command matrices")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    stars = None
    if a.stars is not None:
        if len(a.stars) % 3:
            ap.error("--stars takes triples x y gsalt")
        stars = star_ring(4, a.radius) if not a.stars else [tuple(a.stars[i:i + 3]) for i in range(0, len(a.stars), 3)]
    ps = P.load_param_file(a.config) if a.config.endswith(".py") and os.path.exists(a.config) else P.builtin(a.config)
    far = max([a.radius] + ([np.hypot(x, y) for x, y, _ in stars] if stars else []))
    with_field(ps, far + 5. if a.field is None else a.field)
    sup = VecRlSupervisor(ps, dict(n_reverse_filtered_from_cmat=a.nfilt), a.envs, device=a.device)
    dirs = line(a.radius, a.n)
    print("config %s, %d environments, %d frames, gain %g" % (ps.simul_name, a.envs, a.frames, sup.gain))
    print("%-28s" % "field angle [arcsec]" + "".join("%8.1f" % d[0] for d in dirs) + "   loop's own")
    le, own = strehl_against_angle(sup, dirs, a.frames)
    print("%-28s" % "NGS integrator" + "".join("%8.4f" % v for v in le) + "   %8.4f" % own, flush=True)
    if stars:
        print_tomography(sup, stars, dirs, a.frames)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
