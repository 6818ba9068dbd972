"""Mirror mis-registration per environment: every mirror of every environment seen through its own shift, rotation and
magnification (reference: shesha/supervisor/components/dmCompass.py:148-176, set_dm_registration(dm_index, dx, dy,
theta, G), which hands dx / pixsize, dy / pixsize, theta and G to the native mirror).

The model ("Mirror mis-registration").  On the grid of a source (nn = n for the sensor, pupdiam for the
target; c = (nn - 1) / 2; (ox, oy) the mirror's offset on that grid) environment e and mirror k carry six fp32 numbers
{A00, A01, A10, A11, tx, ty}; pupil pixel (x, y) samples the mirror's plane at

    (u, v) = (c + ox, c + oy) + A (x - c, y - c) + t

by the bilinear rule of the plain ray trace: floor of both coordinates; 0 when the floor cell lies outside [0, dim); the
neighbour index clamped at dim - 1; the value of the cell itself where both weights are zero.  Four-parameter form: the
surface seen in the pupil is the registered one magnified by G about the pupil centre, rotated by theta from x towards
y, then shifted by (dx, dy) pupil pixels: A = (1 / G) [[cos, sin], [-sin, cos]], t = -A (dx, dy).

`trace_model` is that rule in NumPy (float64: the definition; float32: the yardstick of the device's round-off);
`DmRegistration` holds the table of a VecRlSupervisor's simulator (csrc/aomarl_capi_dmreg.hip: k_trace_reg) and, between
start() and stop(), gives VecRlSupervisor.next_part_one its frame (attachments.py: the "registration" row).

    python -m ao_marl_amd.registration <config>      long-exposure Strehl against the shift, nominal and recalibrated
"""
import ctypes as C
import os

import numpy as np

from . import attachments
from .attachments import le_strehl
from .loop_sensor import host_rows, through_mirrors

ROW = 6
A_MAX, DET_MIN, DET_MAX, T_DIMS = 4.0, 0.25, 4.0, 4.0       # csrc/aomarl_dmreg_host.h


# ------------------------------------------------------------------------------------------------ the model
def registration_affine(dx, dy, theta, G, pixsize):
    """(A [..., 2, 2], t [..., 2]) in fp32 of the four parameters (dx, dy in metres, pixsize metres per pupil pixel:
    dmCompass.py:174-175 divides the same way): computed in double, rounded once.  Scalars or arrays of one shape."""
    dx, dy, theta, G = np.broadcast_arrays(*[np.asarray(v, dtype=np.float64) for v in (dx, dy, theta, G)])
    px, py = dx / float(pixsize), dy / float(pixsize)
    c, s = np.cos(theta) / G, np.sin(theta) / G
    A = np.stack([np.stack([c, s], axis=-1), np.stack([-s, c], axis=-1)], axis=-2)
    t = -np.stack([c * px + s * py, -s * px + c * py], axis=-1)
    return A.astype(np.float32), t.astype(np.float32)


def rows_of(A, t):
    """[..., 6] fp32 rows {A00, A01, A10, A11, tx, ty} of A [..., 2, 2] and t [..., 2]"""
    A, t = np.asarray(A, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if A.shape[-2:] != (2, 2) or t.shape[-1:] != (2,) or A.shape[:-2] != t.shape[:-1]:
        raise ValueError("registration: A must be [..., 2, 2] and t [..., 2] (got %s and %s)" % (A.shape, t.shape))
    return np.concatenate([A.reshape(A.shape[:-2] + (4,)), t], axis=-1).astype(np.float32)


IDENTITY_ROW = np.array([1, 0, 0, 1, 0, 0], dtype=np.float32)


def compose_rows(outer, inner):
    """One row for two traces in a row: a plane traced through `inner`, and the result (a plane of the grid's own size
    at offset 0) traced through `outer`, is the plane traced through this row wherever no interpolation and no border
    is involved.  (A, t) = (A_in A_out, A_in t_out + t_in), in float64."""
    o, i = np.asarray(outer, dtype=np.float64), np.asarray(inner, dtype=np.float64)
    Ao, to, Ai, ti = o[:4].reshape(2, 2), o[4:], i[:4].reshape(2, 2), i[4:]
    return np.concatenate([(Ai @ Ao).reshape(4), Ai @ to + ti])


def sample_positions(nn, offset, row, dtype=np.float64):
    """(u, v) [nn, nn] of the grid's pixels (index [y, x]) in the plane of a mirror at `offset` = (ox, oy), in the
    operation order of the kernel (csrc/aomarl_dmreg_host.h: dmreg_sample)."""
    dt = np.dtype(dtype).type
    r = np.asarray(row, dtype=np.float32).astype(dtype)
    c = dt(0.5 * (nn - 1))
    d = np.arange(nn, dtype=dtype) - c
    DX, DY = d[None, :], d[:, None]
    u = (c + dt(offset[0])) + (r[0] * DX + (r[1] * DY + r[4]))
    v = (c + dt(offset[1])) + (r[2] * DX + (r[3] * DY + r[5]))
    return u, v


def bilinear(plane, u, v):
    """The ray trace's bilinear rule at (u, v) (csrc/aomarl_kernels.hip: k_raytrace), in the dtype of u."""
    dt = u.dtype
    plane = np.asarray(plane).astype(dt)
    dim = plane.shape[0]
    one = dt.type(1)
    fu, fv = np.floor(u), np.floor(v)
    ix, iy = fu.astype(np.int64), fv.astype(np.int64)
    inside = (ix >= 0) & (iy >= 0) & (ix < dim) & (iy < dim)
    wx, wy = u - fu, v - fv
    ix0, iy0 = np.clip(ix, 0, dim - 1), np.clip(iy, 0, dim - 1)
    ix1, iy1 = np.minimum(ix0 + 1, dim - 1), np.minimum(iy0 + 1, dim - 1)
    v00, v01, v10, v11 = plane[iy0, ix0], plane[iy0, ix1], plane[iy1, ix0], plane[iy1, ix1]
    val = (one - wy) * ((one - wx) * v00 + wx * v01) + wy * ((one - wx) * v10 + wx * v11)
    val = np.where((wx == 0) & (wy == 0), v00, val)
    return np.where(inside, val, dt.type(0))


def tt_plane(c0, c1, influ, dtype=np.float32):
    """The plane of a tip-tilt mirror as every consumer evaluates it: c0 f0 + c1 f1, influ [dim, dim, 2]."""
    f = np.asarray(influ).astype(dtype)
    dt = np.dtype(dtype).type
    return dt(c0) * f[..., 0] + dt(c1) * f[..., 1]


def trace_model(nn, planes, offsets, rows, dtype=np.float64, start=None):
    """The phase [nn, nn] of the mirrors `planes` (a list of [dim, dim] arrays, controller order; tip-tilt: tt_plane)
    at `offsets` [(ox, oy)] through `rows` [ndm][6] (rounded to fp32 first, as the device holds them), added in
    controller order onto `start` (the atmosphere's part, or what a trace without RESET finds in the buffer)."""
    out = np.zeros((nn, nn), dtype=dtype) if start is None else np.array(start, dtype=dtype)
    for plane, off, row in zip(planes, offsets, rows):
        u, v = sample_positions(nn, off, row, dtype)
        out = out + bilinear(plane, u, v)
    return out


def check_rows(rows, dim, who="DmRegistration.set"):
    """The refusals of aomarl_dmreg_set (csrc/aomarl_dmreg_host.h), by name, before anything reaches the device."""
    r = np.asarray(rows, dtype=np.float32).reshape(-1, ROW)
    if not np.isfinite(r).all():
        raise ValueError(who + ": the table has entries that are not finite")
    if np.abs(r[:, :4]).max() > A_MAX:
        raise ValueError(who + ": |A| entry %g exceeds %g" % (np.abs(r[:, :4]).max(), A_MAX))
    det = np.abs(r[:, 0].astype(np.float64) * r[:, 3] - r[:, 1].astype(np.float64) * r[:, 2])
    if det.min() < DET_MIN or det.max() > DET_MAX:
        bad = det[(det < DET_MIN) | (det > DET_MAX)][0]
        raise ValueError(who + ": |det A| = %g outside [%g, %g] (a magnification G outside [1/2, 2])" % (bad, DET_MIN, DET_MAX))
    if np.abs(r[:, 4:]).max() > T_DIMS * dim:
        raise ValueError(who + ": |t| = %g beyond %g pixels (4 dim of the mirror)" % (np.abs(r[:, 4:]).max(), T_DIMS * dim))
    return r


def trace_bytes(s, target):
    """(bytes one environment's trace moves, bytes shared by all environments), from shapes alone
    (csrc/aomarl_dmreg_host.h: dmreg_trace_bytes): the screens' windows, the mirrors' windows, one store of the grid."""
    nn = s.pupdiam if target else s.n
    b, sh = 4 * nn * nn * s.nscreens + 4 * nn * nn, 0
    for d in s.dms:
        w = min(d.dim, nn)
        if d.type == "pzt":
            b += 4 * w * w
        else:
            b, sh = b + 8, sh + 8 * w * w
    return b, sh


# ------------------------------------------------------------------------------------------------ the native table
class NativeRegistration(object):
    """aomarl_dmreg_* on a HipSim: the device table [nenv][ndm][6] and the registered trace."""

    def __init__(self, sim):
        from . import libaomarl as la
        self.la, self.sim, self.lib = la, sim, sim.lib
        self.h = C.c_void_p()
        la.check(self.lib.aomarl_dmreg_create(sim.ctx, sim.nenv, C.byref(self.h)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.aomarl_dmreg_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_rows(self, dm, rows, env_begin=0):
        r = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, ROW)
        self.la.check(self.lib.aomarl_dmreg_set(self.h, int(env_begin), r.shape[0], int(dm), self.la.fptr(r),
                                                self.sim._stream()))

    def get_rows(self, dm, env_begin=0, env_count=None):
        n = self.sim.nenv - env_begin if env_count is None else env_count
        out = np.empty((max(n, 0), ROW), dtype=np.float32)
        self.la.check(self.lib.aomarl_dmreg_get(self.h, int(env_begin), int(n), int(dm), self.la.fptr(out),
                                                self.sim._stream()))
        return out

    def trace(self, target, atm=True, dms=True, reset=True, mask=False, env_begin=0, env_count=None):
        la, sim = self.la, self.sim
        b, n = sim._range(env_begin, env_count)
        sim._need_phase()
        sim._ensure_shape()
        fl = (la.TRACE_ATMOS if atm else 0) | (la.TRACE_DMS if dms else 0) | (la.TRACE_RESET if reset else 0) | \
            (la.TRACE_MASK if mask else 0)
        la.check(self.lib.aomarl_dmreg_trace(self.h, sim.ctx, C.byref(sim.st), b, n, 1 if target else 0, fl,
                                             sim._stream()))


# ------------------------------------------------------------------------------------------------ the supervisor's side
class DmRegistration(object):
    """The mis-registration of a VecRlSupervisor's mirrors, one (shift, rotation, magnification) per environment and mirror.

        reg = DmRegistration(sup)
        reg.set(0, dx=0.5 * pitch_m)            # or arrays [nenv]; None keeps the last value (dmCompass.py:164-171)
        cmat = reg.calibrate(env=0)             # optional: the command matrix as environment 0's mirrors respond
        reg.start()                             # the supervisor's loop now traces through the table
        ... sup.next_part_one(); sup.next_part_two(...) or VecAoEnv.step (the call-by-call path) ...
        reg.stop()
    """
    slot = "registration"
    row = attachments.TABLE[slot]

    def __init__(self, sup):
        self.sup = sup
        sim, s = sup.sim, sup.s
        self.nenv, self.ndm = int(sim.nenv), len(s.dms)
        self.dims = [int(d.dim) for d in s.dms]
        self.pixsize = float(sup.sysm.geom.pixsize)
        shape = (self.ndm, self.nenv)
        self._p = dict(dx=np.zeros(shape), dy=np.zeros(shape), theta=np.zeros(shape), G=np.ones(shape))
        self.rows = np.tile(IDENTITY_ROW, (self.ndm, self.nenv, 1))          # host copy [ndm][nenv][6]
        self.native = NativeRegistration(sim) if hasattr(sim, "lib") else None
        self._attached = False

    # ---- the table
    def _mirror(self, dm_index, who):
        k = int(dm_index)
        if not 0 <= k < self.ndm:
            raise IndexError("%s: mirror %r of %d" % (who, dm_index, self.ndm))
        return k

    def _per_env(self, v, name, who):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            return np.full(self.nenv, float(a))
        if a.shape != (self.nenv,):
            raise ValueError("%s: %s must be a scalar or one value per environment [%d], got %s" % (who, name, self.nenv, a.shape))
        return a.copy()

    def _store(self, k, rows):
        if self.native is not None:
            self.native.set_rows(k, rows)
        self.rows[k] = rows

    def set(self, dm_index, dx=None, dy=None, theta=None, G=None):
        """dmCompass.set_dm_registration: dx, dy [m], theta [rad], G; scalars or [nenv]; None keeps the last value."""
        who = "DmRegistration.set"
        k = self._mirror(dm_index, who)
        new = {}
        for name, v in (("dx", dx), ("dy", dy), ("theta", theta), ("G", G)):
            new[name] = self._p[name][k] if v is None else self._per_env(v, name, who)
            if not np.isfinite(new[name]).all():
                raise ValueError("%s: %s has entries that are not finite" % (who, name))
        if (new["G"] <= 0).any():
            raise ValueError(who + ": G must be positive")
        A, t = registration_affine(new["dx"], new["dy"], new["theta"], new["G"], self.pixsize)
        rows = check_rows(rows_of(A, t), self.dims[k], who)
        self._store(k, rows)
        for name in new:
            self._p[name][k] = new[name]

    def set_affine(self, dm_index, A, t):
        """The raw map of mirror dm_index: A [2, 2] and t [2] for every environment, or [nenv, 2, 2] and [nenv, 2]
        (pupil pixels).  The four parameters of that mirror read back as NaN afterwards."""
        who = "DmRegistration.set_affine"
        k = self._mirror(dm_index, who)
        rows = rows_of(A, t)
        if rows.ndim == 1:
            rows = np.tile(rows, (self.nenv, 1))
        if rows.shape != (self.nenv, ROW):
            raise ValueError("%s: one map or one per environment [%d], got %s" % (who, self.nenv, rows.shape[:-1]))
        rows = check_rows(rows, self.dims[k], who)
        self._store(k, rows)
        for name in self._p:
            self._p[name][k] = np.nan

    def randomize(self, seed, shift_sigma_m=0.0, theta_sigma=0.0, G_sigma=0.0):
        """Domain randomisation: every (mirror, environment) draws dx, dy ~ N(0, shift_sigma_m), theta ~ N(0,
        theta_sigma), G ~ 1 + N(0, G_sigma) (kept inside [0.55, 1.9]) from ONE numpy Generator seeded with `seed`, in
        the order dx, dy, theta, G, each [ndm][nenv]: the same seed gives the same table."""
        rng = np.random.default_rng(seed)
        shape = (self.ndm, self.nenv)
        dx, dy = rng.normal(0.0, 1.0, shape) * shift_sigma_m, rng.normal(0.0, 1.0, shape) * shift_sigma_m
        th = rng.normal(0.0, 1.0, shape) * theta_sigma
        G = np.clip(1.0 + rng.normal(0.0, 1.0, shape) * G_sigma, 0.55, 1.9)
        for k in range(self.ndm):
            self.set(k, dx=dx[k], dy=dy[k], theta=th[k], G=G[k])

    @property
    def params(self):
        """dict(dx, dy, theta, G: [ndm][nenv] as set (NaN behind set_affine); rows: the table [ndm][nenv][6], read back
        from the device where there is one)"""
        out = {k: v.copy() for k, v in self._p.items()}
        if self.native is not None:
            out["rows"] = np.stack([self.native.get_rows(k) for k in range(self.ndm)])
        else:
            out["rows"] = self.rows.copy()
        return out

    # ---- the trace
    def trace(self, target, atm=True, dms=True, reset=True, env_begin=0, env_count=None):
        """The registered trace into the simulator's phase buffer (sim.t["tar_phase"] / sim.t["wfs_phase"])."""
        if self.native is None:
            raise RuntimeError("DmRegistration.trace: this simulator has no native library; the CPU statement is "
                               "registration.trace_model")
        self.native.trace(target, atm, dms, reset, env_begin=env_begin, env_count=env_count)

    # ---- calibration
    def calibrate(self, env=0, push_um=0.05):
        """The command matrix of the loop as the mirrors of environment `env` respond: every Btt mode pushed and pulled
        by push_um microns rms through comp_dm_shape, the registered trace with the mirrors only and the sensor's
        noise-free image and slopes from the phase buffer, with the rows of `env` on all environments meanwhile; then
        modal.cmat_with_btt with the supervisor's filtered-mode count.  Leaves the table and the mirrors as they were
        (the mirrors on the loop's voltages); installs nothing (install_cmat does)."""
        from . import modal
        sup, sim = self.sup, self.sup.sim
        if self.native is None:
            raise RuntimeError("DmRegistration.calibrate: this simulator has no native library")
        if not 0 <= int(env) < self.nenv:
            raise IndexError("DmRegistration.calibrate: environment %r of %d" % (env, self.nenv))
        m2v = np.asarray(sup.modes2volts, dtype=np.float64)             # [nactu][nmodes]
        v2m = np.asarray(sup.volts2modes, dtype=np.float64)             # [nmodes][nactu]
        keep = self.rows.copy()
        for k in range(self.ndm):
            self.native.set_rows(k, np.tile(keep[k, int(env)], (self.nenv, 1)))

        def read(n):
            self.native.trace(False, atm=False, dms=True, reset=True)
            sim.comp_image(from_phase_buffer=True, noise=False, write_bincube=False, cog=True)
            return host_rows(sim.slopes, n)
        try:
            resp = [through_mirrors(sim, sign * push_um * m2v.T, read) for sign in (1.0, -1.0)]
        finally:
            for k in range(self.ndm):
                self.native.set_rows(k, keep[k])
            sim.comp_dm_shape()                                         # the mirrors back on the loop's voltages
        Dm = ((resp[0] - resp[1]) / (2.0 * push_um)).T                  # [nslope][nmodes]
        self.imat_modes = Dm
        nfilt = max(int(getattr(sup, "n_reverse_filtered_from_cmat", 0)), 0)
        return modal.cmat_with_btt(Dm @ v2m, m2v, nfilt)

    # ---- the loop
    def start(self):
        """Attach: the supervisor's next_part_one traces through this table (see VecRlSupervisor.next_part_one)."""
        attachments.attach(self.sup, self.slot, self)
        self._attached = True
        return self

    def stop(self):
        if self._attached:
            attachments.detach(self.sup, self.slot, self)
            self._attached = False

    def frame(self, move_atmos):
        """The frame of next_part_one behind the move: the unfused frame with both traces through the table (target
        trace and PSF, sensor trace and image, the next move's prefetch).  Returns whether it kept the frame's phase
        copy."""
        sup, sim = self.sup, self.sup.sim
        self.trace(target=True)
        sim.target_psf_buffer()
        self.trace(target=False)
        sim.comp_image(from_phase_buffer=True, noise=True, write_bincube=False, cog=True)
        kept = bool(sup.keep_wfs_phase)
        if kept:                                # the buffer holds the registered phase the sensor just saw
            sup._keep_wfs_phase_buffer()
        if sup.prefetch_atmos and move_atmos:
            sim.prefetch_atmos()
        return kept

    def control(self):
        """The supervisor's own do_control, on its own command matrix (it also feeds an attached control law)."""
        self.sup.sim.do_control()


def install_cmat(sup, cmat):
    """Make `cmat` [nactu][nslope] the supervisor's command matrix (what obtain_and_set_cmat_filtered does with its own)."""
    sup.cal.cmat = cmat
    sup.s.cmat = np.ascontiguousarray(cmat, dtype=np.float32)
    sup.sim.set_cmat(sup.s.cmat)
    sup._s2m_ok = False
    if sup.modal_gains is not None:
        sup.ensure_slopes2modes()


# ------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    import argparse
    from . import params as P
    from .env import VecRlSupervisor
    ap = argparse.ArgumentParser(prog="python -m ao_marl_amd.registration",
                                 description="Long-exposure Strehl of the integrator against a shift of the stack-array "
                                             "mirror, with the nominal and with the recalibrated command matrix")
    ap.add_argument("config", nargs="?", default="production_sh_10x10_2m",
                    help="a built-in configuration or a parameter file (.py)")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--nfilt", type=int, default=5, help="Btt modes filtered from the command matrices")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    ps = P.load_param_file(a.config) if a.config.endswith(".py") and os.path.exists(a.config) else P.builtin(a.config)
    sup = VecRlSupervisor(ps, dict(n_reverse_filtered_from_cmat=a.nfilt), a.envs, device=a.device)
    nominal = np.array(sup.s.cmat, dtype=np.float32)
    reg = DmRegistration(sup)
    pitch_m = float(sup.s.dms[0].pitch) * reg.pixsize
    print("config %s, %d environments, %d frames, gain %g, %d modes filtered, pitch %.4g m (%g pixels)" %
          (ps.simul_name, a.envs, a.frames, sup.gain, a.nfilt, pitch_m, float(sup.s.dms[0].pitch)))
    print("shift [pitch]   LE Strehl nominal cmat   LE Strehl recalibrated cmat")
    for i in range(7):
        shift = 0.1 * i
        reg.set(0, dx=shift * pitch_m)
        recal = reg.calibrate(env=0)
        reg.start()
        install_cmat(sup, nominal)
        sr_nom = le_strehl(sup, a.frames)                  # (the same seeds every row: reset() restarts them)
        install_cmat(sup, recal)
        sr_cal = le_strehl(sup, a.frames)
        reg.stop()
        print("%8.1f        %10.4f             %10.4f" % (shift, sr_nom, sr_cal))
    install_cmat(sup, nominal)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
