"""Laser tomography: a constellation of guide stars on the Shack-Hartmann sensor and an MMSE reconstructor of the on-axis
slopes (learn-and-apply, Vidal et al. 2010, on this simulator's model; the reference has the host wiring alone,
shesha/ao/tomo.py -- its compute_Cmm / compute_Cphim live in an external library that is not in the reference tree).

Layers:
  Constellation, constellation_offsets   the stars (x", y", gsalt; inf: a natural star) and, per (star, layer), the
                                         float32 layer offset and delta - 1 of the trace; every refusal by name
  tomo_trace_model                       lgs.cone_trace_model per star with that star's offsets (NumPy)
  slope_covariance                       the covariance of two-point slopes between directions, float64 NumPy: the
                                         statement k_tomo_cov (csrc/aomarl_tomo.hip) is checked against
  tomo_reconstructor                     R = C_0S (C_SS + diag(noise) + ridge mean(diag C_SS) I)^-1, Cholesky, float64
  LaserTomography(LgsSensor)             the sensor: slot "lgs" of attachments.TABLE, shared with the single star

Model of a slope (slope_covariance): the sub-aperture of side d centred at p, seen from star a through layer l, covers
the layer around u = delta_al p + alt_l theta_a (delta_al = 1 - alt_l / gsalt_a) and its x slope is the difference of the
layer's phase at u +- delta_al d / 2 along x, over d, times kappa = 1e-6 * 206265 (microns over metres to arcsec):
    Cov(s_e^a(i), s_e'^b(j)) = (kappa^2 / d^2) sum_l sum_{s, s' = +-1} (-s s' / 2)
                               D_l(|u_i^{a,l} - u_j^{b,l} + s delta_al d / 2 e - s' delta_bl d / 2 e'|)
(the variances cancel: sum s s' = 0), D_l the von Karman structure function of groot.rodconan at r0_l = r0 /
frac_l^(3/5), in the screens' microns: D_l(r) = rodconan(r, L0_l) r0_l^(-5/3) (0.5 / 2 pi)^2.  Layers outer, then the
four taps (s, s') = (+, +), (+, -), (-, +), (-, -): the order of the sum, on the host and on the device.

Pseudo-open-loop control (`polc`): the stars see S_k = s_k + D v (atmosphere through the cone plus the mirrors, which sit
in the pupil and look alike from every star; D = imat_modes . volts2modes).  The prior is the atmosphere's, so R is
applied to S_k - D v and the mirrors are put back: the on-axis residual is R S - (sum_k R_k - I) D v, and
    err = -cmat_lgs (R S - (sum_k R_k - I) D v) = -cmat_tomo S + G v,   G = cmat_lgs (sum_k R_k - I) D.

    python -m ao_marl_amd.tomography <config> [--stars x y h ...] [--radius arcsec]
"""
import ctypes as C
import os

import numpy as np

from . import geometry as G
from . import libaomarl as la
from . import params as P
from .attachments import le_strehl
from .groot import rodconan
from .lgs import LgsSensor, NativeLgs, _ModelBackend, cone_trace_model
from .loop_sensor import host_rows

__all__ = ["Constellation", "constellation_offsets", "tomo_trace_model", "slope_covariance", "covariance_weight",
           "tomo_reconstructor", "mean_reconstructor", "subap_centres", "atmos_layers", "star_seed_offsets",
           "NativeTomo", "LaserTomography", "MAX_STARS"]

MAX_STARS = 8
KAPPA = 1e-6 * 206265.                  # microns over metres to arcsec
UM_PER_RAD = 0.5 / (2 * np.pi)          # the screens are microns, r0 is given at 0.5 microns
SEED_STRIDE = 0x9E3779B1                # seed of (environment e, star k) = seed_e + (k + 1) SEED_STRIDE mod 2^32


# ------------------------------------------------------------------------------------------------ the constellation
class Constellation(object):
    """stars: [(x", y", gsalt_m), ...], 1 <= K <= 8; gsalt = inf is a natural star (delta = 1 exactly)."""

    def __init__(self, stars):
        try:
            st = [tuple(float(v) for v in s) for s in stars]
        except (TypeError, ValueError):
            raise ValueError("constellation: stars are triples (x arcsec, y arcsec, gsalt m)")
        if not 1 <= len(st) <= MAX_STARS:
            raise ValueError("constellation: %d stars: 1..%d" % (len(st), MAX_STARS))
        for k, s in enumerate(st):
            if len(s) != 3:
                raise ValueError("constellation: star %d: a triple (x arcsec, y arcsec, gsalt m)" % k)
            if not (np.isfinite(s[0]) and np.isfinite(s[1])):
                raise ValueError("constellation: star %d: direction (%r, %r) is not finite" % (k, s[0], s[1]))
            if not s[2] > 0 or np.isnan(s[2]):
                raise ValueError("constellation: star %d: gsalt = %r m must be positive (inf: a natural star)" % (k, s[2]))
        self.stars = st
        self.K = len(st)
        self.xy = np.array([s[:2] for s in st], dtype=np.float64)
        self.gsalt = np.array([s[2] for s in st], dtype=np.float64)

    def deltas(self, alts):
        """delta [K][nlayers]; refuses a star at or below the highest layer, as lgs.cone_deltas does"""
        alts = np.asarray(alts, dtype=np.float64).reshape(-1)
        for k, h in enumerate(self.gsalt):
            if alts.size and h <= alts.max():
                raise ValueError("constellation: star %d: gsalt = %g m is not above the highest layer (%g m)" % (
                    k, h, alts.max()))
        return 1. - alts[None, :] / self.gsalt[:, None]


def _as_constellation(stars):
    return stars if isinstance(stars, Constellation) else Constellation(stars)


def constellation_offsets(sysm, stars, iwfs=0):
    """(off [K][nlayers][2] float32, dm1 [K][nlayers] float32, delta [K][nlayers] float64) of the stars on the system
    `sysm` (geometry.build_system): off_kl = float32(wfs_atm_off_l + theta_k alt_l / pupixsize), dm1_kl = float32(delta_kl
    - 1).  Each star's footprint -- the trace's coordinate at the four corners of the pupil grid -- must lie inside every
    screen (the trace returns 0 outside one)."""
    con = _as_constellation(stars)
    atm, n = sysm.atm, int(sysm.geom.n)
    alt = np.asarray(atm.alt, dtype=np.float64)
    delta = con.deltas(alt)
    base = np.asarray(sysm.wfss[iwfs].atm_off, dtype=np.float64).reshape(alt.size, 2)
    shift = con.xy[:, None, :] * G.ARCSEC2RAD * alt[None, :, None] / float(atm.pupixsize)
    off = (base[None] + shift).astype(np.float32)
    dm1 = (delta - 1.0).astype(np.float32)
    c = 0.5 * (n - 1)
    for k in range(con.K):
        for l in range(alt.size):
            dim = int(atm.dim_screens[l])
            for ax in range(2):
                for x in (0., float(n - 1)):
                    f = (x + float(off[k, l, ax])) + float(dm1[k, l]) * (x - c)
                    if not 0. <= f <= dim - 1:
                        raise ValueError(
                            "constellation: star %d at (%g, %g) arcsec leaves screen %d (%d pixels, altitude %g m): its "
                            "footprint reaches %s = %.2f; the parameter file must declare a field of radius %g arcsec "
                            "(one more entry of p_targets or p_wfss at that radius)" % (
                                k, con.xy[k, 0], con.xy[k, 1], l, dim, alt[l], "xy"[ax], f,
                                np.ceil(np.hypot(con.xy[:, 0], con.xy[:, 1]).max())))
    return off, dm1, delta


def tomo_trace_model(screens, off, deltas, n, dtype=np.float64):
    """planes [K][n][n]: lgs.cone_trace_model of the screens [nlayers][dim][dim] per star with that star's offsets
    off [K][nlayers][2] and deltas [K][nlayers] -- the coordinate ((x, y) + off_kl) + (delta_kl - 1) ((x, y) - c_p)."""
    return np.stack([cone_trace_model(screens, [tuple(o) for o in off[k]], deltas[k], n, dtype=dtype)
                     for k in range(len(off))])


# ------------------------------------------------------------------------------------------------ the covariance
def covariance_weight(d, r0_l):
    """kappa^2 / d^2 r0_l^(-5/3) (0.5 / 2 pi)^2: what multiplies rodconan(r, L0_l) in arcsec^2"""
    return (KAPPA / d)**2 * np.asarray(r0_l, dtype=np.float64)**(-5. / 3.) * UM_PER_RAD**2


def _star_layer(stars, layers):
    con = _as_constellation(stars)
    lay = np.asarray(layers, dtype=np.float64).reshape(-1, 3)
    delta = con.deltas(lay[:, 0])
    shift = con.xy[:, None, :] * G.ARCSEC2RAD * lay[None, :, 0, None]              # [K][nlayers][2] metres
    return con, lay, delta, shift


def slope_covariance(px, py, d, stars_a, stars_b, layers, px_b=None, py_b=None, return_abs=False):
    """The covariance [2 n_a K_a][2 n_b K_b] in arcsec^2 of the two-point slopes (module docstring) of the sub-apertures
    centred at (px, py) metres seen from stars_a (rows) and at (px_b, py_b) -- default the same points -- seen from
    stars_b (columns); x slopes then y slopes per star.  layers: [(alt, r0_l, L0_l), ...].  return_abs: also sum |w D|
    per element, the scale of the round-off of the tap sum."""
    px, py = np.asarray(px, dtype=np.float64).reshape(-1), np.asarray(py, dtype=np.float64).reshape(-1)
    qx = px if px_b is None else np.asarray(px_b, dtype=np.float64).reshape(-1)
    qy = py if py_b is None else np.asarray(py_b, dtype=np.float64).reshape(-1)
    if px.size != py.size or qx.size != qy.size or not px.size or not qx.size:
        raise ValueError("slope_covariance: px / py of equal, positive length")
    if not d > 0:
        raise ValueError("slope_covariance: d = %r m must be positive" % (d,))
    ca, lay, da, sa = _star_layer(stars_a, layers)
    cb, _, db, sb = _star_layer(stars_b, layers)
    if not (np.all(lay[:, 1] > 0) and np.all(lay[:, 2] > 0)):
        raise ValueError("slope_covariance: r0_l and L0_l must be positive")
    na, nb = px.size, qx.size
    out = np.zeros((2 * na * ca.K, 2 * nb * cb.K))
    mag = np.zeros_like(out)
    wl = covariance_weight(d, lay[:, 1])
    axes = ((1., 0.), (0., 1.))
    for a in range(ca.K):
        for b in range(cb.K):
            for ea, (eax, eay) in enumerate(axes):
                for eb, (ebx, eby) in enumerate(axes):
                    acc, am = np.zeros((na, nb)), np.zeros((na, nb))
                    for l in range(lay.shape[0]):
                        ux = (da[a, l] * px + sa[a, l, 0])[:, None] - (db[b, l] * qx + sb[b, l, 0])[None, :]
                        uy = (da[a, l] * py + sa[a, l, 1])[:, None] - (db[b, l] * qy + sb[b, l, 1])[None, :]
                        ha, hb = 0.5 * d * da[a, l], 0.5 * d * db[b, l]
                        for s1 in (1., -1.):
                            for s2 in (1., -1.):
                                x = ux + s1 * ha * eax - s2 * hb * ebx
                                y = uy + s1 * ha * eay - s2 * hb * eby
                                t = (0.5 * wl[l]) * rodconan(np.sqrt(x * x + y * y), lay[l, 2])
                                acc = acc - (s1 * s2) * t
                                am = am + np.abs(t)
                    r0, c0 = (2 * a + ea) * na, (2 * b + eb) * nb
                    out[r0:r0 + na, c0:c0 + nb] = acc
                    mag[r0:r0 + na, c0:c0 + nb] = am
    return (out, mag) if return_abs else out


# ------------------------------------------------------------------------------------------------ the reconstructor
def mean_reconstructor(K, nslope):
    """R = (1 / K) [I ... I]: the stars' mean, the ground-layer baseline"""
    return np.tile(np.eye(nslope) / K, (1, K))


def tomo_reconstructor(C_0S, C_SS, noise_var=0., ridge=1e-6, return_cond=False):
    """R = C_0S (C_SS + diag(noise_var) + ridge mean(diag C_SS) I)^-1 by Cholesky, float64.  Direction 0 is the science
    direction (on axis, delta = 1)."""
    C_0S, C_SS = np.asarray(C_0S, dtype=np.float64), np.asarray(C_SS, dtype=np.float64)
    m = C_SS.shape[0]
    if C_SS.shape != (m, m) or C_0S.ndim != 2 or C_0S.shape[1] != m:
        raise ValueError("tomo_reconstructor: C_0S %r against C_SS %r" % (C_0S.shape, C_SS.shape))
    nv = np.broadcast_to(np.asarray(noise_var, dtype=np.float64), (m,))
    if not np.all(nv >= 0) or not ridge >= 0:
        raise ValueError("tomo_reconstructor: noise_var and ridge must not be negative")
    A = 0.5 * (C_SS + C_SS.T)
    A[np.diag_indices(m)] += nv + ridge * np.mean(np.diag(C_SS))
    from scipy import linalg
    try:
        cf = linalg.cho_factor(A, lower=True)
    except linalg.LinAlgError:
        raise ValueError("tomo_reconstructor: C_SS + noise + ridge is not positive definite (raise ridge = %g)" % ridge)
    R = linalg.cho_solve(cf, C_0S.T).T
    if return_cond:
        ev = np.linalg.eigvalsh(A)
        return R, float(ev[-1] / ev[0])
    return R


# ------------------------------------------------------------------------------------------------ the system's numbers
def subap_centres(s, pupixsize):
    """(px, py) [nvalid] metres of the sub-apertures' centres from the pupil grid's centre, x along the x slopes"""
    pm0 = np.asarray(s.phasemap, dtype=np.int64)[0]
    half = 0.5 * (int(s.pdiam) - 1) - 0.5 * (int(s.n) - 1)
    return ((pm0 % int(s.n)) + half) * float(pupixsize), ((pm0 // int(s.n)) + half) * float(pupixsize)


def atmos_layers(alt, r0, frac, L0):
    """[(alt, r0_l, L0_l)]: r0_l = r0 / frac_l^(3/5), frac normalised to unit sum, as geometry.atmos_geometry has it"""
    alt, L0 = np.asarray(alt, dtype=np.float64).reshape(-1), np.asarray(L0, dtype=np.float64).reshape(-1)
    frac = np.asarray(frac, dtype=np.float64).reshape(-1)
    if not (alt.size == frac.size == L0.size) or not np.all(frac > 0) or not r0 > 0:
        raise ValueError("atmos_layers: alt, frac, L0 of one length, frac and r0 positive")
    frac = frac / frac.sum()
    return np.stack([alt, float(r0) / frac**(3. / 5.), L0], axis=1)


def star_seed_offsets(K):
    """int32 [K]: what is added (mod 2^32) to an environment's seed for star k: (k + 1) SEED_STRIDE"""
    return (((np.arange(K, dtype=np.uint64) + 1) * SEED_STRIDE) & 0xffffffff).astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the device object
class NativeTomo(object):
    """aomarl_tomo_trace / aomarl_tomo_cov (csrc/aomarl_tomo.hip)."""

    def __init__(self, device="cuda:0"):
        import torch
        if not torch.cuda.is_available():
            raise la.AomarlError("NativeTomo needs a GPU (the NumPy statements are tomo_trace_model and slope_covariance)")
        self.lib, self.device = la.load(), torch.device(device)

    def trace(self, sim, off, dm1, planes, atm=True, dms=True, mask=False, env_begin=0, env_count=None):
        """planes: float32 device tensor [nenv][K][n][n] of a HipSim's state through every star's cone (k_tomo_trace)"""
        off = np.ascontiguousarray(off, dtype=np.float32)
        dm1 = np.ascontiguousarray(dm1, dtype=np.float32)
        K, nl = dm1.shape if dm1.ndim == 2 else (0, 0)
        n = sim.nenv - env_begin if env_count is None else int(env_count)
        if tuple(planes.shape) != (sim.nenv, K, sim.s.n, sim.s.n) or str(planes.dtype) != "torch.float32" or \
                not planes.is_cuda or not planes.is_contiguous():
            raise ValueError("planes must be a contiguous float32 device tensor [%d][%d][%d][%d]" % (
                sim.nenv, K, sim.s.n, sim.s.n))
        d = la.TomoDesc()
        d.nstars, d.nlayers, d.off, d.dm1 = K, nl, la.fptr(off), la.fptr(dm1)
        sim._ensure_shape()
        fl = (la.TRACE_ATMOS if atm else 0) | (la.TRACE_DMS if dms else 0) | la.TRACE_RESET | (la.TRACE_MASK if mask else 0)
        la.check(self.lib.aomarl_tomo_trace(sim.ctx, C.byref(sim.st), C.byref(d), planes.data_ptr(), int(env_begin), n, fl,
                                            la.raw_stream(self.device)))
        return planes

    def covariance(self, px, py, d, stars_a, stars_b, layers, px_b=None, py_b=None):
        """slope_covariance on the device (k_tomo_cov): a float64 device tensor [2 n_a K_a][2 n_b K_b]"""
        import torch
        f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)  # noqa: E731
        ca, cb = _as_constellation(stars_a), _as_constellation(stars_b)
        lay = f64(np.asarray(layers, dtype=np.float64).reshape(-1, 3))
        ca.deltas(lay[:, 0]), cb.deltas(lay[:, 0])
        px, py = f64(px).reshape(-1), f64(py).reshape(-1)
        qx, qy = (px if px_b is None else f64(px_b).reshape(-1)), (py if py_b is None else f64(py_b).reshape(-1))
        if px.size != py.size or qx.size != qy.size:
            raise ValueError("covariance: px / py of equal length")
        sa, sb = f64(np.array(ca.stars)), f64(np.array(cb.stars))
        dd = la.TomoCovDesc()
        dd.n_row, dd.n_col, dd.k_row, dd.k_col, dd.nlayers, dd.d = px.size, qx.size, ca.K, cb.K, lay.shape[0], float(d)
        dd.row_px, dd.row_py, dd.col_px, dd.col_py = la.dptr(px), la.dptr(py), la.dptr(qx), la.dptr(qy)
        dd.row_stars, dd.col_stars, dd.layers = la.dptr(sa), la.dptr(sb), la.dptr(lay)
        out = torch.zeros(2 * px.size * ca.K, 2 * qx.size * cb.K, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_tomo_cov(C.byref(dd), out.data_ptr(), la.raw_stream(self.device)))
        return out


# ------------------------------------------------------------------------------------------------ the sensor
class LaserTomography(LgsSensor):
    """A constellation of guide stars on a VecRlSupervisor's Shack-Hartmann system with a tomographic reconstructor of
    the on-axis slopes.  It is an LGS sensor: slot "lgs" of attachments.TABLE, that row's refusals and messages.

        tomo = LaserTomography(sup, stars=[(20, 0, 90e3), (0, 20, 90e3), (-20, 0, 90e3), (0, -20, 90e3)])
        tomo.calibrate()        # flat reference, cmat_lgs, the covariances, R, cmat_tomo, G
        tomo.start() ... tomo.stop()

    reconstructor: "tomo" (MMSE) or "mean" (the stars' mean: the ground-layer baseline).  One launch telescope and one
    elongation kernel set for all stars; gsalt of the kernels and of the photometry is LgsSensor's argument `gsalt`
    (default: the lowest finite star).  Seeds: star k of environment e draws with seed_e + (k + 1) 0x9E3779B1 mod 2^32;
    the frame counter is the simulator's, handed to every star before the measure and taken back from star 0 behind it.
    `slopes` / get_slopes() is the on-axis estimate R S [nenv][nslope]; `star_slopes` is S [nenv][K nslope]."""
    keeps_phase = False                 # the simulator's buffer is not the stars': the supervisor traces its own copy

    def __init__(self, sup, stars, llt=None, reconstructor="tomo", polc=True, noise_var=None, ridge=1e-6, **kw):
        if reconstructor not in ("tomo", "mean"):
            raise ValueError("LaserTomography: reconstructor %r ('tomo' or 'mean')" % (reconstructor,))
        self.con = _as_constellation(stars)
        self.K = self.con.K
        finite = self.con.gsalt[np.isfinite(self.con.gsalt)]
        if kw.get("gsalt") is None:
            kw["gsalt"] = float(finite.min()) if finite.size else 1e9
        self.off, self.dm1, self.star_deltas = constellation_offsets(sup.sysm, self.con)
        self._nenv_real = int(sup.sim.nenv)
        LgsSensor.__init__(self, sup, llt=llt, **kw)          # (the mirror-at-altitude refusal is the parent's)
        self.reconstructor, self.polc, self.noise_var, self.ridge = reconstructor, bool(polc), noise_var, float(ridge)
        s = self.s
        nenv, K, n = self._nenv_real, self.K, int(s.n)
        nz = self.native.noise
        # the measuring object over K nenv pseudo-environments: pseudo-environment e K + k is star k of environment e
        if self.device == "cpu" or str(self.device) == "cpu":
            self.native = _ModelBackend(s, nenv * K, self.kernels, self.nphotons, nz)
            self.tomo = None
            self.planes = np.zeros((nenv, K, n, n))
            self.est = np.zeros((nenv, self.nslope))
        else:
            import torch
            self.native = NativeLgs(s, nenv * K, self.kernels, self.nphotons, nz, device=sup.sim.device)
            self.tomo = NativeTomo(sup.sim.device)
            f32 = dict(dtype=torch.float32, device=self.device)
            self.planes = torch.zeros(nenv, K, n, n, **f32)
            self.est = torch.zeros(nenv, self.nslope, **f32)
            self._seeds = torch.zeros(nenv, K, dtype=torch.int32, device=self.device)
            self._frames = torch.zeros(nenv, K, dtype=torch.int32, device=self.device)
            self._koff = torch.as_tensor(star_seed_offsets(K), device=self.device).reshape(1, K)
        self.nenv = nenv
        pix = float(sup.sysm.atm.pupixsize)
        self.px, self.py = subap_centres(s, pix)
        self.subapd = float(s.subapd)
        a, pa = sup.sysm.atm, sup.config.p_atmos
        self.alt = np.asarray(a.alt, dtype=np.float64)
        self.set_prior(float(pa.r0), np.asarray(pa.frac, dtype=np.float64), np.asarray(pa.L0, dtype=np.float64))
        self.R = self.cmat_tomo = self.G = self.cond = self.cmat_lgs = self.D = self.star_match = None
        self.noise_var_used = None
        self._dev = None

    def set_prior(self, r0, frac, L0):
        self.layers = atmos_layers(self.alt, r0, frac, L0)

    # ---- measurements
    @property
    def slopes(self):
        return self.est

    @property
    def star_slopes(self):
        return self.native.slopes.reshape(self.nenv, self.K * self.nslope)

    def trace(self, atm=True, dms=True, env_begin=0, env_count=None):
        """Every star's pupil phase of the simulator's state, into `planes` [nenv][K][n][n]."""
        sim = self.sup.sim
        if self.tomo is not None:
            self.tomo.trace(sim, self.off, self.dm1, self.planes, atm, dms, False, env_begin, env_count)
            return
        sims = getattr(sim, "sims", None)
        if sims is None:
            raise NotImplementedError("the constellation's trace on the CPU needs a simulator with one oracle per "
                                      "environment (`sims`); tomo_trace_model is the NumPy statement")
        n = self.nenv - env_begin if env_count is None else int(env_count)
        for e in range(env_begin, env_begin + n):
            o = sims[e]
            self.planes[e] = tomo_trace_model(o.screens, self.off, self.star_deltas, self.s.n, dtype=np.float32) if atm else 0.
            if dms:
                o.raytrace_wfs(atm=False, dms=True, reset=True)
                self.planes[e] += np.asarray(o.wfs_phase, dtype=np.float64)[None]

    def measure(self, phase=None, noise=None, env_begin=0, env_count=None, write_cube=True):
        """Slopes of all stars of `phase` [nenv][K][n][n] (default: `planes`, as `trace` left them); returns S
        [nenv][K nslope]."""
        sim, K = self.sup.sim, self.K
        ph = self.planes if phase is None else phase
        ph = ph.reshape(self.nenv * K, self.s.n, self.s.n)
        n = self.nenv - env_begin if env_count is None else int(env_count)
        noisy = (self.native.noise >= 0) if noise is None else bool(noise)
        if noisy and self.tomo is None:
            raise NotImplementedError("measure: noise uses the device simulator's seeds and frame counters")
        if noisy:
            self._seeds.copy_(sim.t["seeds"].reshape(self.nenv, 1).expand(self.nenv, K))
            self._seeds.add_(self._koff)
            self._frames.copy_(sim.t["frame"].reshape(self.nenv, 1).expand(self.nenv, K))
        self.native.measure(ph, noisy, self._seeds.reshape(-1) if noisy else None,
                            self._frames.reshape(-1) if noisy else None, env_begin * K, n * K, write_cube)
        if noisy and self.native.noise >= 0:
            sim.t["frame"][env_begin:env_begin + n].copy_(self._frames[env_begin:env_begin + n, 0])
        return self.star_slopes

    def estimate(self, S=None):
        """R S: the on-axis slopes [..][nslope] of the stars' slopes S [..][K nslope] (default: the last measure's),
        float64 on the host"""
        if self.R is None:
            raise RuntimeError("estimate: calibrate() first")
        S = host_rows(self.star_slopes, self.nenv) if S is None else np.asarray(S, dtype=np.float64)
        return S @ self.R.T

    # ---- what LoopSensor asks for
    def _quiet(self):
        self.trace(atm=False, dms=True)
        self.measure(noise=False, write_cube=False)

    def _trace(self):
        self.trace()

    def _measure(self):
        self.measure(write_cube=False)

    def _star_rows(self, nn, k=0):
        """the slopes of star k of the first nn environments, float64 on the host"""
        return host_rows(self.native.slopes.reshape(self.nenv, self.K, self.nslope)[:, k], nn)

    def _response(self, volts):
        def read(nn):
            self._quiet()
            return self._star_rows(nn)
        return self._mirrors_only(volts, read)

    # ---- calibration
    def covariances(self):
        """(C_0S [nslope][K nslope], C_SS [K nslope][K nslope]) float64 on the host: on the device when there is one"""
        args = (self.px, self.py, self.subapd)
        science = [(0., 0., np.inf)]
        if self.tomo is not None:
            c0 = self.tomo.covariance(*args, science, self.con, self.layers).cpu().numpy()
            cs = self.tomo.covariance(*args, self.con, self.con, self.layers).cpu().numpy()
            return c0, cs
        return slope_covariance(*args, science, self.con, self.layers), slope_covariance(*args, self.con, self.con, self.layers)

    def _flat_noise_var(self, rounds=4):
        """the variance [K nslope] of the sensor's own noisy measurements of the flat mirrors (0 without noise)"""
        if self.native.noise < 0 or self.tomo is None:
            return np.zeros(self.K * self.nslope)
        sim = self.sup.sim
        keep = sim.t["frame"].clone()
        sim.comp_dm_shape(self._volts(np.zeros((1, self.s.nactu))))
        self.trace(atm=False, dms=True)
        rows = []
        for _ in range(rounds):
            self.measure(noise=True, write_cube=False)
            rows.append(host_rows(self.star_slopes, self.nenv))
        sim.t["frame"].copy_(keep)
        return np.concatenate(rows).var(axis=0)

    def calibrate(self, push_um=0.01):
        """The parent's calibration on star 0 (flat reference, cmat_lgs), then the covariances from the system's
        atmosphere, R, cmat_tomo = cmat_lgs R [nactu][K nslope] and G = cmat_lgs (sum_k R_k - I) D [nactu][nactu].
        Returns cmat_tomo."""
        cmat_lgs = np.asarray(LgsSensor.calibrate(self, push_um), dtype=np.float64)
        sup = self.sup
        m2v = np.asarray(sup.modes2volts, dtype=np.float64)
        v2m = np.asarray(sup.volts2modes, dtype=np.float64)
        # with the mirrors in the pupil every star responds alike: one pushed mode, all stars
        sup.sim.comp_dm_shape(self._volts((m2v[:, :1] * self.push[0]).T))
        self._quiet()
        rows = np.stack([self._star_rows(1, k)[0] for k in range(self.K)])
        self.star_match = float(np.abs(rows - rows[:1]).max() / max(np.abs(rows[0]).max(), 1e-300))
        if not self.star_match <= 1e-3:
            raise RuntimeError("LaserTomography.calibrate: the stars' responses to one pushed mode differ by %.3g of the "
                               "response: the mirrors are not in the pupil" % self.star_match)
        nv = self._flat_noise_var() if self.noise_var is None else self.noise_var
        sim = sup.sim
        if str(sim.device) == "cpu":
            sim.comp_dm_shape(np.asarray(sim.voltage)[:, :m2v.shape[0]])
        else:
            sim.comp_dm_shape()
        self.cmat_lgs, self.D = cmat_lgs, self.imat_modes @ v2m
        self.noise_var_used = nv
        self._solve()
        return self.cmat_tomo

    def _solve(self):
        K, ns = self.K, self.nslope
        if self.reconstructor == "mean":
            self.R, self.cond = mean_reconstructor(K, ns), 1.0
        else:
            c0, cs = self.covariances()
            self.R, self.cond = tomo_reconstructor(c0, cs, self.noise_var_used, self.ridge, return_cond=True)
        Rsum = self.R.reshape(ns, K, ns).sum(axis=1)
        self.cmat_tomo = self.cmat_lgs @ self.R
        self.G = self.cmat_lgs @ (Rsum - np.eye(ns)) @ self.D
        if self._dev is not None:                               # attached or started before: the same buffers, rewritten
            import torch
            for t, a in zip(self._dev, (self.cmat_tomo, self.R, self._g_padded())):
                t.copy_(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)))

    def set_reconstructor(self, reconstructor=None, polc=None):
        """Switch between "tomo" and "mean" and the pseudo-open-loop term on the same calibration (values left out
        stay); the loop may be running."""
        if reconstructor is not None and reconstructor not in ("tomo", "mean"):
            raise ValueError("LaserTomography: reconstructor %r ('tomo' or 'mean')" % (reconstructor,))
        if self.cmat_lgs is None:
            raise RuntimeError("set_reconstructor: calibrate() first")
        self.polc = self.polc if polc is None else bool(polc)
        if reconstructor is not None and reconstructor != self.reconstructor:
            self.reconstructor = reconstructor
            self._solve()

    def _g_padded(self):
        """G with zero columns up to the width of the simulator's voltage buffer: the product reads the buffer whole"""
        ld = int(self.sup.sim._frame_buf("voltage").shape[1])
        return np.pad(self.G, ((0, 0), (0, ld - self.G.shape[1])))

    def set_atmosphere(self, r0=None, frac=None, L0=None):
        """Recompute R, cmat_tomo and G for a changed prior (values left out stay); the loop may be running."""
        if self.cmat_lgs is None:
            raise RuntimeError("set_atmosphere: calibrate() first")
        lay = self.layers
        cur_frac = lay[:, 1]**(-5. / 3.)
        cur_r0 = float((cur_frac.sum())**(-3. / 5.))
        self.set_prior(cur_r0 if r0 is None else float(r0), cur_frac / cur_frac.sum() if frac is None else frac,
                       lay[:, 2] if L0 is None else np.broadcast_to(np.asarray(L0, dtype=np.float64), lay[:, 2].shape))
        self._solve()
        return self.R

    # ---- the loop
    def start(self):
        if self.cmat_tomo is None and self.cmat is not None:
            raise RuntimeError(self.row.who + ": calibrate() first (a constellation needs its reconstructor)")
        LgsSensor.start(self)
        if self.tomo is not None and self._dev is None:
            import torch
            self._dev = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=self.device)
                         for a in (self.cmat_tomo, self.R, self._g_padded())]
        return self

    def control(self):
        """est = R S; err = -cmat_tomo S (+ G voltage with polc); com += gain err."""
        sup, sim = self.sup, self.sup.sim
        if self.tomo is not None:
            ct, R, Gm = self._dev
            S = self.star_slopes
            sim.gemm_nt(S, R, alpha=1.0, beta=0.0, Cout=self.est)
            sim.gemm_nt(S, ct, alpha=-1.0, beta=0.0, Cout=sim.err)
            if self.polc:
                sim.gemm_nt(sim._frame_buf("voltage"), Gm, alpha=1.0, beta=1.0, Cout=sim.err)
            sim.com.add_(sim.err, alpha=float(sup.gain))
            return
        S = np.asarray(self.star_slopes, dtype=np.float64)
        self.est[:] = S @ self.R.T
        na = self.cmat_tomo.shape[0]
        for e, o in enumerate(sim.sims):
            err = -(self.cmat_tomo @ S[e])
            if self.polc:
                err = err + self.G @ np.asarray(o.voltage, dtype=np.float64)[:na]
            o.err[:na] = err.astype(np.float32)
            o.com[:na] += np.float32(sup.gain) * o.err[:na]


# ------------------------------------------------------------------------------------------------ command line
def ring(K, radius, gsalt=90e3):
    """K stars at `gsalt` on a circle of `radius` arcsec, the first on the x axis"""
    a = 2 * np.pi * np.arange(K) / K
    return [(float(round(radius * np.cos(t), 9)), float(round(radius * np.sin(t), 9)), float(gsalt)) for t in a]


def with_field(ps, radius):
    """`ps` with one more p_targets entry at `radius` arcsec on the x axis: it declares the field, so that
    geometry.atmos_geometry sizes the screens for it (the loop's target stays p_targets[0])"""
    import copy
    t = copy.deepcopy(ps.p_targets[0])
    t.xpos, t.ypos = float(radius), 0.
    ps.p_targets = list(ps.p_targets) + [t]
    return ps


def main(argv=None):
    import argparse
    from .env import VecRlSupervisor
    ap = argparse.ArgumentParser(prog="python -m ao_marl_amd.tomography",
                                 description="Long-exposure Strehl on the same seeds: the NGS integrator, one on-axis LGS, "
                                             "the constellation with the stars' mean and with the MMSE reconstructor "
                                             "(with and without the pseudo-open-loop term)")
    ap.add_argument("config", nargs="?", default="production_sh_10x10_2m",
                    help="a built-in configuration or a parameter file (.py)")
    ap.add_argument("--stars", type=float, nargs="+", default=None, metavar="V",
                    help="x y gsalt per star (default: 4 stars at 90 km on a circle of --radius)")
    ap.add_argument("--radius", type=float, default=20., help="arcsec")
    ap.add_argument("--field", type=float, default=None, help="the declared field radius in arcsec (default: radius + 5)")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--nfilt", type=int, default=5, help="Btt modes filtered from the command matrices")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.stars is not None and (len(a.stars) % 3 or not a.stars):
        ap.error("--stars takes triples x y gsalt")
    stars = ring(4, a.radius) if a.stars is None else [tuple(a.stars[i:i + 3]) for i in range(0, len(a.stars), 3)]
    ps = P.load_param_file(a.config) if a.config.endswith(".py") and os.path.exists(a.config) else P.builtin(a.config)
    far = max(np.hypot(x, y) for x, y, _ in stars)
    with_field(ps, far + 5. if a.field is None else a.field)
    sup = VecRlSupervisor(ps, dict(n_reverse_filtered_from_cmat=a.nfilt), a.envs, device=a.device)
    print("config %s, %d environments, %d frames, gain %g, stars %s" % (ps.simul_name, a.envs, a.frames, sup.gain, stars))
    print("long-exposure Strehl  NGS integrator                     %.4f" % le_strehl(sup, a.frames))
    one = LgsSensor(sup, gsalt=min(h for _, _, h in stars if np.isfinite(h)) if any(np.isfinite(h) for _, _, h in stars)
                    else 90e3)
    one.calibrate()
    one.start()
    print("long-exposure Strehl  one on-axis LGS                    %.4f" % le_strehl(sup, a.frames))
    one.stop()
    for rec, polc in (("mean", False), ("tomo", True), ("tomo", False)):
        t = LaserTomography(sup, stars, reconstructor=rec, polc=polc)
        t.calibrate()
        t.start()
        sr = le_strehl(sup, a.frames)
        t.stop()
        print("long-exposure Strehl  constellation, %-4s%-16s %.4f   (cond %.3g)" % (
            rec, ", polc" if polc else "", sr, t.cond))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
