"""Multi-conjugate AO: stack-array mirrors conjugated to altitude on the constellation of laser tomography, driven together
with the system's own mirrors by one least-squares reconstructor over all stars.  In the reference the same system is an
`ls` controller over several sensors and several mirrors with p_dm.alt > 0 (shesha/init/dm_init.py: _dm_init with alt > 0,
rtc_init.py: imat over every sensor); here the altitude mirrors belong to the attachment, the way the stars belong to
LaserTomography -- the parameter file's own mirrors stay what they are (modal.correct_dm would cut a mirror at altitude
down to its on-axis footprint).

Layers:
  altitude_mirror       geometry.pzt_geometry for p_dm.alt > 0 on an integer pitch: the lattice, the separable profile
  mirror_shape_model    commands -> the mirror's plane, float64 NumPy: the statement k_mcao_shape is checked against
  mirror_offsets        per (star or direction, mirror): the float32 offset and -h / gsalt of the sampling rule; refusals
  mirrors_add_model     planes += the mirrors sampled by that rule: the statement k_mcao_add is checked against
  delay_line_model      the delay line of aomarl_apply_control, float32
  ls_reconstructor      truncated, ridged pseudo-inverse of the interaction matrix
  NativeMcao            aomarl_mcao_* (csrc/aomarl_mcao.hip)
  MultiConjugate        the attachment: a LaserTomography (slot "lgs" of attachments.TABLE) that owns 1 or 2 mirrors

The sampling rule: pixel (x, y) of a grid of side nn samples mirror m for star k at
    ((x, y) + off_km) + dm1_km ((x, y) - (nn - 1) / 2),      off_km = theta_k h_m / pupixsize + (dim_m - n) / 2 (+ pupdiff),
    dm1_km = -h_m / gsalt_k  (0: a natural star, a science direction),
one fused multiply-add per coordinate -- the layer rule of tomography.constellation_offsets --, bilinear by the trace's
rule for a plain plane: zero outside, the last line clamped.

    python -m ao_marl_amd.mcao <config> [--stars x y gsalt ...] [--alt h ...] [--radius arcsec] [--frames F]
"""
import ctypes as C
import os

import numpy as np

from . import attachments
from . import geometry as G
from . import libaomarl as la
from .loop_sensor import host_rows
from .tomography import LaserTomography, _as_constellation

__all__ = ["altitude_mirror", "mirror_shape_model", "mirror_offsets", "sample_model", "mirrors_add_model",
           "delay_weights_f32", "delay_line_model", "ls_reconstructor", "mcao_desc", "NativeMcao", "MultiConjugate", "MAX_MIRRORS",
           "MAX_DIRS"]

MAX_MIRRORS = 2                         # AOMARL_MCAO_MAX_MIRRORS
MAX_DIRS = 8                            # AOMARL_MCAO_MAX_DIRS
SHAPE_TILE, SHAPE_CELLS, SHAPE_MAX_SS = 32, 12, 128       # k_mcao_shape (csrc/aomarl_mcao_host.h)


# ------------------------------------------------------------------------------------------------ the mirror
def altitude_mirror(sysm, alt, field_radius, pitch=None, coupling=0.2, unitpervolt=None):
    """A stack-array mirror conjugated to `alt` metres that covers a field of radius `field_radius` arcsec on the system
    `sysm` (geometry.build_system): geometry.pzt_geometry for p_dm.alt > 0 -- the Rigaut profile, cobs = 0, every actuator
    within rad_out kept, no correct_dm -- with one deviation: the pitch is an integer number of pixels (default: the
    system's own stack-array pitch) and the actuator count follows from it, nact = ceil(patch / pitch) + 1, centred on the
    plane; the reference derives a fractional pitch from nact.  The plane has an even side `dim`, just large enough for
    every kept actuator's patch; its centre (dim - 1) / 2 lies under the centre of the pupil grid.
    Returns a Bag: alt, pitch, nact, dim, i1min, j1min (the lattice origin: the patch of cell (gx, gy) starts at
    (i1min + pitch gx, j1min + pitch gy)), gw, gh, grid [gh][gw] (actuator index or -1), ss, prof [ss] (float64, separable:
    influence(a, b) = prof[a] prof[b] microns per unit command), ntotact, i1, j1, xpos, ypos (pixels of the plane)."""
    alt, field_radius = float(alt), float(field_radius)
    if not alt >= 0 or not np.isfinite(alt):
        raise ValueError("altitude_mirror: alt = %r m: finite and not negative" % (alt,))
    if not field_radius >= 0 or not np.isfinite(field_radius):
        raise ValueError("altitude_mirror: field_radius = %r arcsec: finite and not negative" % (field_radius,))
    if not 0 < coupling < 1:
        raise ValueError("altitude_mirror: coupling = %r must lie in (0, 1)" % (coupling,))
    own = [d for d in sysm.dms if d.type == "pzt"]
    if pitch is None:
        if not own or float(own[0].pitch) != int(own[0].pitch):
            raise ValueError("altitude_mirror: the system's stack-array pitch is not a whole number of pixels; pass pitch")
        pitch = int(own[0].pitch)
    if int(pitch) != pitch or pitch < 1:
        raise ValueError("altitude_mirror: pitch = %r: a whole number of pixels" % (pitch,))
    pitch = int(pitch)
    if unitpervolt is None:
        unitpervolt = float(own[0].unitpervolt) if own else 0.01
    if not unitpervolt > 0:
        raise ValueError("altitude_mirror: unitpervolt = %r must be positive" % (unitpervolt,))
    pupdiam, pix = int(sysm.geom.pupdiam), float(sysm.atm.pupixsize)
    patch = pupdiam + 2 * field_radius * G.ARCSEC2RAD * alt / pix
    nact = int(np.ceil(patch / pitch)) + 1
    ss, prof = G.rigaut_size_and_profile(pitch, coupling)
    nx = nact + 4
    g = np.arange(nx) - (nx - 1.) / 2.
    gx, gy = np.tile(g, nx), np.repeat(g, nx)
    rad_out = ((nact - 1.) / 2. + 1.44) * pitch                  # (margin_out's default; cobs = 0: no inner radius)
    sel = np.where(np.hypot(gx, gy) * pitch <= rad_out)[0]
    half = int(np.ceil(np.abs(np.concatenate([gx[sel], gy[sel]])).max() * pitch + ss / 2 + 1))
    dim = 2 * half
    cent = dim / 2 + 0.5                                         # the reference's 1-based frame: pixel i is i + 1, n1 = 1
    xpos, ypos = gx[sel] * pitch + cent, gy[sel] * pitch + cent
    i1 = (xpos - ss / 2 - 0.5 - 1).astype(np.int64)
    j1 = (ypos - ss / 2 - 0.5 - 1).astype(np.int64)
    k = np.arange(ss, dtype=np.float64)
    fx = prof((i1[None, :] + k[:, None]) + 1. - xpos[None, :])              # [ss][act]
    fy = prof((j1[None, :] + k[:, None]) + 1. - ypos[None, :])
    if np.abs(fx - fx[:, :1]).max() != 0 or np.abs(fy - fx[:, :1]).max() != 0:
        raise RuntimeError("altitude_mirror: the actuators' patches differ: the lattice is not regular")   # (never: integer pitch)
    p = fx[:, 0] / fx[:, 0].max() * np.sqrt(unitpervolt)
    i1min, j1min = int(i1.min()), int(j1.min())
    gw, gh = int((i1.max() - i1min) // pitch + 1), int((j1.max() - j1min) // pitch + 1)
    grid = np.full((gh, gw), -1, dtype=np.int32)
    grid[(j1 - j1min) // pitch, (i1 - i1min) // pitch] = np.arange(sel.size, dtype=np.int32)
    if i1min < 0 or j1min < 0 or i1.max() + ss > dim or j1.max() + ss > dim:
        raise RuntimeError("altitude_mirror: the lattice leaves the plane")                                  # (never: dim is sized for it)
    return G.Bag(alt=alt, pitch=pitch, nact=nact, dim=dim, i1min=i1min, j1min=j1min, gw=gw, gh=gh, grid=grid, ss=int(ss),
                 prof=p, ntotact=int(sel.size), i1=i1, j1=j1, xpos=xpos - 1., ypos=ypos - 1., patch=patch,
                 coupling=float(coupling), unitpervolt=float(unitpervolt), field_radius=field_radius)


def mirror_shape_model(mirror, com, dtype=np.float64):
    """[...][ntotact] -> [...][dim][dim]: shape[y][x] = sum_act com[act] prof[x - i1_act] prof[y - j1_act], in the microns of
    dm_shape.  Evaluated through the lattice, C[gy][gx] = com[grid[gy][gx]] (0 for an empty cell): P^T C P with
    P[g][x] = prof[x - (i1min + pitch g)].  dtype np.float32: the same statement in single precision."""
    dt = np.dtype(dtype)
    com = np.asarray(com, dtype=dt)
    if com.shape[-1] != mirror.ntotact:
        raise ValueError("mirror_shape_model: %d commands for %d actuators" % (com.shape[-1], mirror.ntotact))
    lead = com.shape[:-1]
    Cg = np.zeros(lead + (mirror.gh * mirror.gw,), dtype=dt)
    flat = mirror.grid.reshape(-1)
    Cg[..., flat >= 0] = com[..., flat[flat >= 0]]
    Cg = Cg.reshape(lead + (mirror.gh, mirror.gw))

    def taps(g0, ng):
        P = np.zeros((ng, mirror.dim), dtype=dt)
        for gi in range(ng):
            P[gi, g0 + mirror.pitch * gi:g0 + mirror.pitch * gi + mirror.ss] = mirror.prof.astype(dt)
        return P
    Px, Py = taps(mirror.i1min, mirror.gw), taps(mirror.j1min, mirror.gh)
    rows = np.matmul(Cg, Px).astype(dt)                                    # [...][gh][dim]
    return np.matmul(np.swapaxes(Py, 0, 1), rows).astype(dt)              # [...][dim][dim]


# ------------------------------------------------------------------------------------------------ who looks, and how
def _lookers(stars_or_directions):
    """(xy [K][2] arcsec, gsalt [K] m): triples (x, y, gsalt) are guide stars, pairs (x, y) science directions (gsalt inf)"""
    if hasattr(stars_or_directions, "gsalt"):
        return stars_or_directions.xy, stars_or_directions.gsalt
    try:
        rows = [tuple(float(v) for v in p) for p in stars_or_directions]
    except (TypeError, ValueError):
        raise ValueError("mirror_offsets: stars are triples (x, y, gsalt), directions pairs (x, y), in arcsec and metres")
    if not rows or len({len(r) for r in rows}) != 1 or len(rows[0]) not in (2, 3):
        raise ValueError("mirror_offsets: stars are triples (x, y, gsalt), directions pairs (x, y), in arcsec and metres")
    if len(rows[0]) == 3:
        con = _as_constellation(rows)
        return con.xy, con.gsalt
    xy = np.array(rows, dtype=np.float64)
    for k, p in enumerate(xy):
        if not np.all(np.isfinite(p)):
            raise ValueError("mirror_offsets: direction %d: (%g, %g) is not finite" % (k, p[0], p[1]))
    return xy, np.full(len(rows), np.inf)


def mirror_offsets(sysm, mirrors, stars_or_directions, grid="wfs"):
    """(off [K][M][2] float32, dm1 [K][M] float32) of the stars (triples, or a tomography.Constellation) or science
    directions (pairs, relative to the target) on the mirrors: off = theta_k ARCSEC2RAD h_m / pupixsize + (dim_m - n) / 2,
    plus pupdiff = (n - pupdiam) / 2 on the pupil grid; dm1 = -h_m / gsalt_k, 0 for a natural star and for every science
    direction.  grid: "wfs" (side n, theta relative to the sensor's guide star) or "pupil" (side pupdiam, theta relative to
    p_targets[0]).  Each footprint -- the coordinate at the grid's corners, as the kernel evaluates it -- must lie inside
    the mirror's plane [0, dim_m - 1]."""
    if grid not in ("wfs", "pupil"):
        raise ValueError("mirror_offsets: grid %r ('wfs' or 'pupil')" % (grid,))
    xy, gsalt = _lookers(stars_or_directions)
    n, pupdiam, pix = int(sysm.geom.n), int(sysm.geom.pupdiam), float(sysm.atm.pupixsize)
    ps = sysm.params
    base = ps.p_wfss[0] if grid == "wfs" else ps.p_targets[0]
    theta = xy + np.array([float(getattr(base, "xpos", 0.) or 0.), float(getattr(base, "ypos", 0.) or 0.)])[None]
    nn = n if grid == "wfs" else pupdiam
    pupdiff = 0. if grid == "wfs" else 0.5 * (n - pupdiam)
    K, M = len(xy), len(mirrors)
    off, dm1 = np.zeros((K, M, 2), dtype=np.float32), np.zeros((K, M), dtype=np.float32)
    c = 0.5 * (nn - 1)
    for m, mir in enumerate(mirrors):
        for k in range(K):
            if np.isfinite(gsalt[k]) and not gsalt[k] > mir.alt:
                raise ValueError("mirror_offsets: star %d: gsalt = %g m is not above mirror %d (%g m)" % (k, gsalt[k], m, mir.alt))
            off[k, m] = theta[k] * G.ARCSEC2RAD * mir.alt / pix + 0.5 * (mir.dim - n) + pupdiff
            dm1[k, m] = 0.0 - mir.alt / gsalt[k]
            for ax in range(2):
                for x in (0., nn - 1.):
                    f = (x + float(off[k, m, ax])) + float(dm1[k, m]) * (x - c)
                    if not 0. <= f <= mir.dim - 1:
                        raise ValueError(
                            "mirror_offsets: %s %d at (%g, %g) arcsec leaves mirror %d (%d pixels, altitude %g m): its "
                            "footprint reaches %s = %.2f; build the mirror for a field radius of %g arcsec" % (
                                "star" if grid == "wfs" else "direction", k, xy[k, 0], xy[k, 1], m, mir.dim, mir.alt,
                                "xy"[ax], f, np.ceil(np.hypot(theta[:, 0], theta[:, 1]).max())))
    return off, dm1


def sample_model(shape, off, dm1, nn, dtype=np.float64):
    """[nn][nn]: the plane `shape` [dim][dim] sampled at ((x, y) + off) + dm1 ((x, y) - (nn - 1) / 2), bilinear, zero
    outside, the last line clamped.  np.float32: the arithmetic of the device's kernel, the position one fused
    multiply-add, the taps (1 - w) v0 + w v1 along x, then along y."""
    dt = np.dtype(dtype).type
    shape = np.asarray(shape, dtype=dt)
    dim = shape.shape[0]
    xs = np.arange(nn).astype(dt)
    c, m = dt(0.5 * (nn - 1)), dt(dm1)

    def pos(o):
        base = xs + dt(o)
        if dt is np.float32:                 # fma(m, x - c, x + o): one rounding
            return (base.astype(np.float64) + np.float64(m) * (xs - c).astype(np.float64)).astype(np.float32)
        return base + m * (xs - c)
    fx, fy = pos(off[0]), pos(off[1])
    ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    wx, wy = (fx - ix.astype(dt)).astype(dt), (fy - iy.astype(dt)).astype(dt)
    okx, oky = (ix >= 0) & (ix < dim), (iy >= 0) & (iy < dim)
    ixc, iyc = np.clip(ix, 0, dim - 1), np.clip(iy, 0, dim - 1)
    ix1, iy1 = np.minimum(ixc + 1, dim - 1), np.minimum(iyc + 1, dim - 1)
    one = dt(1)
    top = (one - wx)[None, :] * shape[iyc][:, ixc] + wx[None, :] * shape[iyc][:, ix1]
    bot = (one - wx)[None, :] * shape[iy1][:, ixc] + wx[None, :] * shape[iy1][:, ix1]
    v = (one - wy)[:, None] * top + wy[:, None] * bot
    return np.where(oky[:, None] & okx[None, :], v, dt(0)).astype(dt)


def mirrors_add_model(planes, shapes, off, dm1, dtype=None):
    """planes [...][K][nn][nn] += sum_m sample_model(shapes[m] [...][dim_m][dim_m]) with off [K][M][2] and dm1 [K][M], in
    mirror order, after whatever the plane holds (in place; returns planes).  dtype: the arithmetic (default: the
    planes')."""
    dt = planes.dtype if dtype is None else np.dtype(dtype)
    K, nn = planes.shape[-3], planes.shape[-1]
    lead = planes.shape[:-3]
    for idx in np.ndindex(*lead):
        for k in range(K):
            acc = planes[idx + (k,)].astype(dt)
            for m, sh in enumerate(shapes):
                acc = (acc + sample_model(sh[idx], off[k, m], dm1[k, m], nn, dt)).astype(dt)
            planes[idx + (k,)] = acc
    return planes


# ------------------------------------------------------------------------------------------------ the delay line
def delay_weights_f32(delay):
    """(wa, wb, wc) float32 of voltage = wa com + wb com1 + wc com2: delay_weights(delay, false) of the library"""
    d = np.float32(delay)
    one, two = np.float32(1), np.float32(2)
    return (one - d, d, np.float32(0)) if d <= one else (np.float32(0), two - d, d - one)


def delay_line_model(coms, delay, state=None):
    """The voltages [T][...] of the command series coms [T][...]: per frame voltage = wa com + wb com1 + wc com2 in float32,
    then com2 <- com1, com1 <- com -- aomarl_apply_control's order (k_delay).  state: (com1, com2) to start from and
    updated in place (default: zeros)."""
    coms = np.asarray(coms, dtype=np.float32)
    wa, wb, wc = delay_weights_f32(delay)
    c1, c2 = (np.zeros_like(coms[0]), np.zeros_like(coms[0])) if state is None else state
    out = np.zeros_like(coms)
    for t in range(coms.shape[0]):
        out[t] = wa * coms[t] + wb * c1 + wc * c2
        c2[...] = c1
        c1[...] = coms[t]
    return out


# ------------------------------------------------------------------------------------------------ the reconstructor
def ls_reconstructor(D, maxcond=None, ridge=0., return_svd=False, equilibrate=False):
    """W [ncol][nrow] of the interaction matrix D [nrow][ncol]: the SVD D = U diag(s) V^T, the singular values below
    s_max / maxcond cut (maxcond None: none but exact zeros), the kept ones filtered with the Tikhonov term
    lam = ridge mean(s_kept^2): W = V_k diag(s / (s^2 + lam)) U_k^T.  equilibrate: the SVD is that of D with its columns
    scaled to unit Euclidean norm (columns in different units -- modes and actuators -- then weigh alike in the cut) and W's
    rows are scaled back.  Returns (W, ncut) -- with return_svd also (s, V^T)."""
    D = np.asarray(D, dtype=np.float64)
    if equilibrate:
        nrm = np.linalg.norm(D, axis=0)
        nrm = np.where(nrm > 0, nrm, 1.)
        out = ls_reconstructor(D / nrm[None, :], maxcond, ridge, return_svd)
        return (out[0] / nrm[:, None],) + tuple(out[1:])
    if D.ndim != 2 or not np.all(np.isfinite(D)):
        raise ValueError("ls_reconstructor: D must be a finite matrix")
    if maxcond is not None and not maxcond >= 1:
        raise ValueError("ls_reconstructor: maxcond = %r: at least 1, or None" % (maxcond,))
    if not ridge >= 0:
        raise ValueError("ls_reconstructor: ridge = %r must not be negative" % (ridge,))
    U, s, Vt = np.linalg.svd(D, full_matrices=False)
    floor = s[0] / maxcond if maxcond is not None else s[0] * max(D.shape) * np.finfo(np.float64).eps
    keep = s >= floor
    keep &= s > 0
    sk = s[keep]
    lam = ridge * np.mean(sk**2) if sk.size else 0.
    W = (Vt[keep].T * (sk / (sk**2 + lam))[None, :]) @ U[:, keep].T
    ncut = int(s.size - sk.size)
    return (W, ncut, s, Vt) if return_svd else (W, ncut)


# ------------------------------------------------------------------------------------------------ the device object
class _DeviceView(object):
    """a device buffer the library owns, as the array interface torch.as_tensor reads"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


def mcao_desc(mirrors):
    """(aomarl_mcao_desc of the mirrors, the arrays it points to: keep them alive as long as the desc is used)"""
    d, keep = la.McaoDesc(), []
    d.nmirrors = len(mirrors)
    for m, mir in enumerate(mirrors[:la.MCAO_MAX_MIRRORS]):
        grid = np.ascontiguousarray(mir.grid, dtype=np.int32)
        prof = np.ascontiguousarray(mir.prof, dtype=np.float32)
        keep += [grid, prof]
        D = d.mirrors[m]
        D.alt, D.dim, D.pitch, D.i1min, D.j1min = float(mir.alt), int(mir.dim), int(mir.pitch), int(mir.i1min), int(mir.j1min)
        D.gw, D.gh, D.ss, D.nact = int(mir.gw), int(mir.gh), int(mir.ss), int(mir.ntotact)
        D.grid, D.prof = la.iptr(grid), la.fptr(prof)
    return d, keep


class NativeMcao(object):
    """aomarl_mcao_* (csrc/aomarl_mcao.hip) on a HipSim's context.  `com`, `voltage` [nenv][nact_total] and `planes`
    [nenv][M][dim_max^2] are views of the buffers the object owns: they live as long as it does."""

    def __init__(self, sim, mirrors):
        import torch
        if not torch.cuda.is_available():
            raise la.AomarlError("NativeMcao needs a GPU (the NumPy statements are mirror_shape_model and mirrors_add_model)")
        self.lib, self.sim, self.device = la.load(), sim, sim.device
        self.mirrors = list(mirrors)
        self.M, self.nenv = len(self.mirrors), int(sim.nenv)
        d, self._keep = mcao_desc(self.mirrors)
        self.dims = [int(mir.dim) for mir in self.mirrors]
        self.nact_total = sum(int(mir.ntotact) for mir in self.mirrors)
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_mcao_create(sim.ctx, self.nenv, C.byref(d), C.byref(self.handle)))
            com, volt, pl = C.c_void_p(), C.c_void_p(), C.c_void_p()
            la.check(self.lib.aomarl_mcao_com(self.handle, C.byref(com), C.byref(volt), C.byref(pl)))
            self.stride = max(self.dims)**2
            self.com = torch.as_tensor(_DeviceView(com.value, (self.nenv, self.nact_total)), device=self.device)
            self.voltage = torch.as_tensor(_DeviceView(volt.value, (self.nenv, self.nact_total)), device=self.device)
            self.planes = torch.as_tensor(_DeviceView(pl.value, (self.nenv, self.M, self.stride)), device=self.device)

    def _stream(self):
        return la.raw_stream(self.device)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                import torch
                torch.cuda.synchronize(self.device)
                self.lib.aomarl_mcao_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _n(self, env_begin, env_count):
        return self.nenv - env_begin if env_count is None else int(env_count)

    mc = property(lambda self: self)            # (what a ScienceField asks of its `mirrors`: mirrors, mc, alt_shapes)

    def alt_shapes(self):
        return [self.plane(m) for m in range(self.M)]

    def plane(self, m):
        """mirror m's plane [nenv][dim_m][dim_m]: a view"""
        d = self.dims[m]
        return self.planes[:, m, :d * d].reshape(self.nenv, d, d)

    def apply(self, volts=None, env_begin=0, env_count=None):
        """volts None: the delay line, then the planes from the voltages; volts [env_count][nact_total] (a float32 device
        tensor): shaped directly"""
        n = self._n(env_begin, env_count)
        ptr = None
        if volts is not None:
            if tuple(volts.shape) != (n, self.nact_total) or str(volts.dtype) != "torch.float32" or not volts.is_cuda or \
                    not volts.is_contiguous():
                raise ValueError("volts must be a contiguous float32 device tensor [%d][%d]" % (n, self.nact_total))
            ptr = volts.data_ptr()
        la.check(self.lib.aomarl_mcao_apply(self.handle, self.sim.ctx, int(env_begin), n, ptr, self._stream()))

    def reset(self, env_begin=0, env_count=None):
        la.check(self.lib.aomarl_mcao_reset(self.handle, int(env_begin), self._n(env_begin, env_count), self._stream()))

    def view(self, off, dm1):
        """an aomarl_mcao_view of off [K][M][2], dm1 [K][M] (the arrays are kept alive by the returned tuple)"""
        off = np.ascontiguousarray(off, dtype=np.float32)
        dm1 = np.ascontiguousarray(dm1, dtype=np.float32)
        v = la.McaoView()
        v.ndir, v.off, v.dm1 = int(dm1.shape[0]) if dm1.ndim == 2 else 0, la.fptr(off), la.fptr(dm1)
        return v, off, dm1

    def add(self, off, dm1, planes, mask=False, env_begin=0, env_count=None):
        """planes: a contiguous float32 device tensor [nenv][K][nn][nn] ([nenv][nn][nn] with one direction)"""
        n = self._n(env_begin, env_count)
        if planes.dim() == 3:
            planes = planes.unsqueeze(1)
        if planes.dim() != 4 or planes.shape[0] != self.nenv or planes.shape[2] != planes.shape[3] or \
                str(planes.dtype) != "torch.float32" or not planes.is_cuda or not planes.is_contiguous():
            raise ValueError("planes must be a contiguous float32 device tensor [%d][K][nn][nn]" % self.nenv)
        v = self.view(off, dm1)
        la.check(self.lib.aomarl_mcao_add(self.handle, self.sim.ctx, C.byref(v[0]), planes.data_ptr(), int(planes.shape[1]),
                                          int(planes.shape[2]), int(env_begin), n, la.TRACE_MASK if mask else 0, self._stream()))
        return planes


# ------------------------------------------------------------------------------------------------ the attachment
class MultiConjugate(LaserTomography):
    """Laser tomography's constellation with 1 or 2 stack-array mirrors conjugated to altitude, owned by the attachment.

        mc = MultiConjugate(sup, stars, mirrors=[(8000.,)], field_radius=25.)
        cg, ca = mc.calibrate()       # flat reference, Btt modes on every star, every altitude actuator poked, the ls matrix
        mc.start() ... mc.stop()

    mirrors: per mirror (alt,), (alt, pitch) or (alt, pitch, coupling) -- altitude_mirror's arguments -- or a Bag it
    returned.  reconstructor "ls": one least-squares reconstructor over all stars drives the ground modes and the altitude
    actuators; "mean": the parent's ground-layer baseline with the altitude mirrors at rest.  maxcond: the singular values
    of the interaction matrix D = [modes | altitude actuators] WITH ITS COLUMNS SCALED TO UNIT NORM that lie below
    s_max / maxcond are cut (the modes' columns are in Btt units, the actuators' in commands of 0.01 microns: on D as it
    stands the cut would compare units); ridge: Tikhonov term ridge mean(s^2) on the kept ones (ls_reconstructor with
    equilibrate=True).  There is no pseudo-open-loop term: polc is refused.  Every guide star, the loop's
    science target and (ScienceField(..., mirrors=mc), or mc.field(directions)) every science direction see the mirrors.
    Agents keep acting on the ground modes (rl_control); the altitude mirrors run the integrator.
    `slopes` / get_slopes() is the stars' mean [nenv][nslope]; `alt_com`, `alt_voltage` [nenv][nact_total]."""
    altitude_mirrors = True

    def __init__(self, sup, stars, mirrors=((8000.,),), field_radius=25., reconstructor="ls", maxcond=10., ridge=1e-3,
                 llt=None, **kw):
        if reconstructor not in ("ls", "mean"):
            raise ValueError("MultiConjugate: reconstructor %r ('ls' or 'mean')" % (reconstructor,))
        mirrors = list(mirrors)
        if not 1 <= len(mirrors) <= MAX_MIRRORS:
            raise ValueError("MultiConjugate: %d mirrors: 1..%d" % (len(mirrors), MAX_MIRRORS))
        if maxcond is not None and not maxcond >= 1:
            raise ValueError("MultiConjugate: maxcond = %r: at least 1, or None" % (maxcond,))
        self.mirrors = [m if hasattr(m, "grid") else altitude_mirror(sup.sysm, m[0], field_radius, *m[1:]) for m in mirrors]
        for m in self.mirrors:
            if m.ss > SHAPE_MAX_SS or (SHAPE_TILE + m.ss - 2) // m.pitch + 2 > SHAPE_CELLS:
                raise ValueError("MultiConjugate: a profile of ss = %d pixels at pitch %d is larger than the shape kernel's "
                                 "LDS patch (%d lattice cells per axis, ss <= %d)" % (m.ss, m.pitch, SHAPE_CELLS, SHAPE_MAX_SS))
        if kw.pop("polc", False):
            raise NotImplementedError("MultiConjugate: polc: the ls reconstructor has no pseudo-open-loop term")
        LaserTomography.__init__(self, sup, stars, llt=llt, reconstructor="mean", polc=False, ridge=ridge, **kw)
        self.reconstructor, self.maxcond = reconstructor, maxcond
        self.M = len(self.mirrors)
        self.nact_alt = [int(m.ntotact) for m in self.mirrors]
        self.nact_total = int(sum(self.nact_alt))
        self.wfs_view = mirror_offsets(sup.sysm, self.mirrors, self.con, "wfs")
        self.sci_view = mirror_offsets(sup.sysm, self.mirrors, [(0., 0.)], "pupil")
        nenv = self.nenv
        if self.tomo is not None:
            import torch
            self.mc = NativeMcao(sup.sim, self.mirrors)
            self._alt_err = torch.zeros(nenv, self.nact_total, dtype=torch.float32, device=self.device)
        else:
            self.mc = None
            self._com = np.zeros((nenv, self.nact_total), dtype=np.float32)
            self._com1, self._com2, self._volt = (np.zeros_like(self._com) for _ in range(3))
            self._shapes = [np.zeros((nenv, m.dim, m.dim), dtype=np.float32) for m in self.mirrors]
        self.cmat_ground = self.cmat_alt = self.D_alt = self.D_ls = self.ncut = self.svals = None
        self._ls_dev = None

    # ---- the altitude mirrors' state
    @property
    def alt_com(self):
        return self.mc.com if self.mc is not None else self._com

    @property
    def alt_voltage(self):
        return self.mc.voltage if self.mc is not None else self._volt

    def alt_shapes(self):
        """the mirrors' planes: per mirror [nenv][dim_m][dim_m] (device: views)"""
        return [self.mc.plane(m) for m in range(self.M)] if self.mc is not None else self._shapes

    def _split(self, v):
        o, out = 0, []
        for n in self.nact_alt:
            out.append(v[..., o:o + n])
            o += n
        return out

    def shape_commands(self, volts, env_begin=0, env_count=None):
        """The planes of the commands volts [env_count][nact_total], directly (no delay line): the calibration's pokes"""
        if self.mc is not None:
            import torch
            self.mc.apply(torch.as_tensor(np.ascontiguousarray(volts, dtype=np.float32), device=self.device)
                          if isinstance(volts, np.ndarray) else volts, env_begin, env_count)
            return
        volts = np.asarray(volts, dtype=np.float32)
        for m, v in enumerate(self._split(volts)):
            self._shapes[m][env_begin:env_begin + volts.shape[0]] = mirror_shape_model(self.mirrors[m], v, np.float32)

    def apply(self):
        """Behind the simulator's apply_control (the supervisor's next_part_two calls it): the altitude mirrors' delay line
        and planes."""
        if self.mc is not None:
            self.mc.apply()
            return
        self._volt[:] = delay_line_model(self._com[None], self.s.delay, (self._com1, self._com2))[0]
        self.shape_commands(self._volt)

    def reset(self):
        """Behind the simulator's reset (the supervisor's reset calls it): commands, delay line, voltages and planes zero."""
        if self.mc is not None:
            self.mc.reset()
            return
        for a in [self._com, self._com1, self._com2, self._volt] + self._shapes:
            a[...] = 0

    # ---- measurements
    def trace(self, atm=True, dms=True, env_begin=0, env_count=None):
        """The parent's trace, then the altitude mirrors on the same planes (with dms)."""
        LaserTomography.trace(self, atm, dms, env_begin, env_count)
        if not dms:
            return
        off, dm1 = self.wfs_view
        if self.mc is not None:
            self.mc.add(off, dm1, self.planes, False, env_begin, env_count)
            return
        n = self.nenv - env_begin if env_count is None else int(env_count)
        sl = slice(env_begin, env_begin + n)
        self.planes[sl] = mirrors_add_model(self.planes[sl], [s[sl] for s in self._shapes], off, dm1, np.float32)

    def frame(self, move_atmos):
        """The frame of next_part_one behind the move: the target's trace, the altitude mirrors on it (one direction, on
        axis), the PSF of that buffer; then the stars."""
        sup, sim = self.sup, self.sup.sim
        off, dm1 = self.sci_view
        if self.mc is not None:
            sim.raytrace_target()
            self.mc.add(off, dm1, sim.t["tar_phase"])
            sim.target_psf_buffer()
        else:
            for e, o in enumerate(sim.sims):
                o.raytrace_target()
                pl = np.asarray(o.tar_phase, dtype=np.float32)[None].copy()
                o.tar_phase[:] = mirrors_add_model(pl, [s[e] for s in self._shapes], off, dm1, np.float32)[0]
        self._trace()
        if sup.prefetch_atmos and move_atmos:
            sim.prefetch_atmos()
        self._measure()
        return False

    # ---- calibration
    def _alt_response(self, volts):
        """Noise-free slopes [P][K nslope] (float64, host) of the altitude commands volts [P][nact_total], the atmosphere off
        and the system's mirrors flat, nenv pokes per call"""
        rows = []
        for k0 in range(0, volts.shape[0], self.nenv):
            chunk = np.zeros((self.nenv, self.nact_total), dtype=np.float32)
            nn = min(self.nenv, volts.shape[0] - k0)
            chunk[:nn] = volts[k0:k0 + nn]
            self.shape_commands(chunk)
            self.trace(atm=False, dms=True)
            self.measure(noise=False, write_cube=False)
            rows.append(host_rows(self.star_slopes, nn))
        return np.concatenate(rows)

    def calibrate(self, push_um=0.01, push_alt_um=0.05):
        """The parent's calibration with the stars' mean (flat reference, the Btt modes through the system's mirrors,
        `star_match`), then every altitude actuator pushed and pulled by push_alt_um microns at its peak and read on all K
        stars: D_alt [K nslope][nact_total].  D = [D_modes | D_alt] with D_modes the kept Btt modes' responses, the same
        on every star.  "ls": W = ls_reconstructor(D, maxcond, ridge); the ground rows are m2v_kept W_modes, the altitude
        rows W_alt.  "mean": the parent's matrix, the altitude rows zero.  `ncut`: the singular values cut.
        Returns (cmat_ground [nactu][K nslope], cmat_alt [nact_total][K nslope])."""
        from . import modal
        if not push_alt_um > 0:
            raise ValueError("calibrate: push_alt_um = %r must be positive" % (push_alt_um,))
        sup, sim = self.sup, self.sup.sim
        self.reset()                                             # the altitude mirrors at rest under the parent's pushes
        keep, self.reconstructor = self.reconstructor, "mean"
        try:
            LaserTomography.calibrate(self, push_um)
        finally:
            self.reconstructor = keep
        K, ns = self.K, self.nslope
        m2v = np.asarray(sup.modes2volts, dtype=np.float64)
        nfilt = max(int(getattr(sup, "n_reverse_filtered_from_cmat", 0)), 0)
        m2v_kept = modal._btt_filtered(m2v, nfilt)                                   # [nactu][nm]
        D_modes = np.tile(self.imat_modes @ modal._btt_filtered(np.eye(m2v.shape[1]), nfilt), (K, 1))   # [K ns][nm]
        # the altitude actuators, the system's mirrors flat
        sim.comp_dm_shape(self._volts(np.zeros((1, m2v.shape[0]))))
        a = np.concatenate([np.full(m.ntotact, push_alt_um / m.prof.max()**2) for m in self.mirrors])
        pokes = np.diag(a)
        self.D_alt = ((self._alt_response(pokes) - self._alt_response(-pokes)) / (2 * a[:, None])).T       # [K ns][nact_total]
        self.shape_commands(np.zeros((self.nenv, self.nact_total), dtype=np.float32))
        if str(sim.device) == "cpu":
            sim.comp_dm_shape(np.asarray(sim.voltage)[:, :m2v.shape[0]])
        else:
            sim.comp_dm_shape()
        self.D_ls = np.concatenate([D_modes, self.D_alt], axis=1)
        self._m2v_kept = m2v_kept
        return self.solve()

    def solve(self, maxcond=False, ridge=None):
        """The matrices again from the calibration's D with another maxcond / ridge (values left out stay); the loop may be
        running.  Returns (cmat_ground, cmat_alt)."""
        if self.D_ls is None:
            raise RuntimeError("solve: calibrate() first")
        if maxcond is not False:
            if maxcond is not None and not maxcond >= 1:
                raise ValueError("MultiConjugate: maxcond = %r: at least 1, or None" % (maxcond,))
            self.maxcond = maxcond
        self.ridge = self.ridge if ridge is None else float(ridge)
        nm = self._m2v_kept.shape[1]
        if self.reconstructor == "ls":
            W, self.ncut, self.svals, _ = ls_reconstructor(self.D_ls, self.maxcond, self.ridge, return_svd=True, equilibrate=True)
            self.cmat_ground, self.cmat_alt = self._m2v_kept @ W[:nm], W[nm:].copy()
        else:
            self.ncut, self.svals = 0, None
            self.cmat_ground, self.cmat_alt = self.cmat_tomo.copy(), np.zeros((self.nact_total, self.K * self.nslope))
        if self._ls_dev is not None:
            self._upload()
        return self.cmat_ground, self.cmat_alt

    def set_reconstructor(self, reconstructor=None, polc=None):
        raise NotImplementedError("MultiConjugate: the reconstructor is chosen at construction; calibrate() solves it")

    def set_atmosphere(self, r0=None, frac=None, L0=None):
        raise NotImplementedError("MultiConjugate: set_atmosphere: neither reconstructor has a prior of the atmosphere "
                                  "(an MMSE reconstructor for the altitude mirrors is not built)")

    def _upload(self):
        import torch
        mats = [np.ascontiguousarray(a, dtype=np.float32) for a in (self.cmat_ground, self.cmat_alt)]
        if self._ls_dev is None:
            self._ls_dev = [torch.as_tensor(a, device=self.device) for a in mats]
        else:
            for t, a in zip(self._ls_dev, mats):
                t.copy_(torch.as_tensor(a))

    # ---- the loop
    def start(self):
        if self.cmat_ground is None:
            raise RuntimeError(self.row.who + ": calibrate() first (the altitude mirrors need their reconstructor)")
        attachments.refuse(self.sup, self.row.who, (("keep_image", "the full-frame image's own trace does not see the mirrors "
                                                     "at altitude"),))
        if getattr(self.sup, "keep_wfs_phase", False):
            raise RuntimeError(self.row.who + ": keep_wfs_phase: the supervisor's copy of the sensor's phase does not see the "
                               "mirrors at altitude")
        LaserTomography.start(self)
        if self.mc is not None:
            self._upload()
        return self

    def control(self):
        """est = the stars' mean; err = -cmat_ground S, com += gain err; alt_com += gain (-cmat_alt S)."""
        sup, sim = self.sup, self.sup.sim
        if self.reconstructor == "mean":
            return LaserTomography.control(self)
        g = float(sup.gain)
        if self.mc is not None:
            import torch
            cg, ca = self._ls_dev
            S = self.star_slopes
            torch.mean(S.view(self.nenv, self.K, self.nslope), dim=1, out=self.est)
            sim.gemm_nt(S, cg, alpha=-1.0, beta=0.0, Cout=sim.err)
            sim.com.add_(sim.err, alpha=g)
            sim.gemm_nt(S, ca, alpha=-1.0, beta=0.0, Cout=self._alt_err)
            self.mc.com.add_(self._alt_err, alpha=g)
            return
        S = np.asarray(self.star_slopes, dtype=np.float64)
        self.est[:] = S.reshape(self.nenv, self.K, self.nslope).mean(axis=1)
        na = self.cmat_ground.shape[0]
        for e, o in enumerate(sim.sims):
            o.err[:na] = (-(self.cmat_ground @ S[e])).astype(np.float32)
            o.com[:na] += np.float32(g) * o.err[:na]
            self._com[e] += np.float32(g) * (-(self.cmat_alt @ S[e])).astype(np.float32)

    def field(self, directions, Lambda=None):
        """A ScienceField on the same supervisor that sees the altitude mirrors"""
        from .field import ScienceField
        return ScienceField(self.sup, directions, Lambda=Lambda, mirrors=self)


# ------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    import argparse
    from . import params as P
    from .env import VecRlSupervisor
    from .field import line, print_tomography, strehl_against_angle
    from .tomography import ring, with_field
    ap = argparse.ArgumentParser(prog="python -m ao_marl_amd.mcao",
                                 description="Long-exposure Strehl against the field angle on the same seeds: the NGS "
                                             "integrator, laser tomography (the stars' mean and the MMSE reconstructor with "
                                             "the pseudo-open-loop term) and multi-conjugate AO with the ls reconstructor")
    ap.add_argument("config", nargs="?", default="production_sh_10x10_2m",
                    help="a built-in configuration or a parameter file (.py)")
    ap.add_argument("--stars", type=float, nargs="+", default=None, metavar="V",
                    help="x y gsalt per star (default: 4 stars at 90 km on a circle of --radius)")
    ap.add_argument("--alt", type=float, nargs="+", default=[8000.], metavar="H", help="the mirrors' altitudes in metres (1 or 2)")
    ap.add_argument("--layers", type=float, nargs="+", default=None, metavar="H",
                    help="the layers' altitudes in place of the file's (equal fractions)")
    ap.add_argument("--radius", type=float, default=20., help="arcsec: the directions run from the target out to it")
    ap.add_argument("--n", type=int, default=5, help="directions along the line")
    ap.add_argument("--field", type=float, default=None, help="the declared field radius in arcsec (default: radius + 5)")
    ap.add_argument("--maxcond", type=float, nargs="+", default=[10.], help="one MCAO row per value")
    ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--mcao-only", action="store_true", help="skip the rows of the NGS integrator and of laser tomography")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--nfilt", type=int, default=5, help="Btt modes filtered from the command matrices")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.stars is not None and (len(a.stars) % 3 or not a.stars):
        ap.error("--stars takes triples x y gsalt")
    if not 1 <= len(a.alt) <= MAX_MIRRORS:
        ap.error("--alt takes 1 or %d altitudes" % MAX_MIRRORS)
    stars = ring(4, a.radius) if a.stars is None else [tuple(a.stars[i:i + 3]) for i in range(0, len(a.stars), 3)]
    ps = P.load_param_file(a.config) if a.config.endswith(".py") and os.path.exists(a.config) else P.builtin(a.config)
    if a.layers is not None:
        at, k = ps.p_atmos, len(a.layers)
        first = lambda v: np.asarray(v).reshape(-1)[0]  # noqa: E731
        at.nscreens, at.alt, at.frac = k, np.asarray(a.layers, dtype=np.float64), np.full(k, 1.0 / k)
        at.windspeed, at.winddir = np.full(k, float(first(at.windspeed))), np.full(k, float(first(at.winddir)))
        at.L0 = np.full(k, float(first(at.L0)))
    far = max([a.radius] + [np.hypot(x, y) for x, y, _ in stars])
    fr = far + 5. if a.field is None else a.field
    with_field(ps, fr)
    sup = VecRlSupervisor(ps, dict(n_reverse_filtered_from_cmat=a.nfilt), a.envs, device=a.device)
    dirs = line(a.radius, a.n)
    print("config %s, %d environments, %d frames, gain %g, layers %s m, mirrors at %s m" % (
        ps.simul_name, a.envs, a.frames, sup.gain, list(np.asarray(ps.p_atmos.alt).reshape(-1)), a.alt))
    print("%-28s" % "field angle [arcsec]" + "".join("%8.1f" % d[0] for d in dirs) + "   loop's own")
    if not a.mcao_only:
        le, own = strehl_against_angle(sup, dirs, a.frames)
        print("%-28s" % "NGS integrator" + "".join("%8.4f" % v for v in le) + "   %8.4f" % own, flush=True)
        print_tomography(sup, stars, dirs, a.frames)
    for mcnd in a.maxcond:
        mc = MultiConjugate(sup, stars, mirrors=[(h,) for h in a.alt], field_radius=fr, maxcond=mcnd, ridge=a.ridge)
        mc.calibrate()
        mc.start()
        try:
            le, own = strehl_against_angle(sup, dirs, a.frames, mirrors=mc)
        finally:
            mc.stop()
        print("%-28s" % ("MCAO ls, maxcond %g" % mcnd) + "".join("%8.4f" % v for v in le) + "   %8.4f   (%d of %d cut)" % (
            own, mc.ncut, mc.svals.size), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
