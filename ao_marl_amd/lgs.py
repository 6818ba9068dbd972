"""Laser guide star on a Shack-Hartmann sensor: spots elongated by the sodium layer's depth, and the cone effect.

Four layers:
  lgs_kernels       the elongation kernel K[nvalid][N][N] of every sub-aperture, host only, float64
  LgsModel          the definition of the image and the slopes, NumPy, float64 (or float32: the yardstick of the device's
                    error); the CPU path.  cone_trace_model is the NumPy statement of the cone trace.
  NativeLgs         aomarl_lgs_* (csrc/aomarl_lgs.hip): the same model on the GPU in fp32
  LgsSensor         an LGS on the guide star of a VecRlSupervisor's NGS Shack-Hartmann system: calibration (`calibrate`)
                    and the closed loop (`start` / `stop`: the supervisor's next_part_one then traces through the cone,
                    measures the elongated spots and integrates err = -cmat_lgs . slopes)

The host side of the reference is shesha/init/lgs_init.py (make_lgs_prof1d / prep_lgs_prof) and the LGS branches of
wfs_init.py:170-185, geom_init.py:391-392 and geom_init.py:751; the image formation and the trace themselves are not in
the reference tree.  What is stated here and not pinned by the reference's Python is listed in DESIGN.md ("Laser guide
star").

Kernel of sub-aperture k (lgs_kernels):
  xsubs = linspace((d - D) / 2, (D - d) / 2, nxsub), d = D / nxsub;  (x, y) = xsubs[validsubsx_k // npix],
  xsubs[validsubsy_k // npix];  r_k = hypot(x - lltx, y - llty), az_k = arctan2(y - llty, x - lltx);
  hG = sum h prof / sum prof;  a sodium bin at altitude h lies at u = (h - hG) 206265 r_k / hG^2 arcsec along the
  elongation axis;  the profile is integrated into cells of width qpixsize / 2 along u (masses m_j, centres u_j:
  np.diff(np.interp(edges, cell edges of h, cumulative profile)), the reference's resampling);  the beam is a Gaussian
  of sigma = beamsize / 2.35482005 in both axes:
      K_k(iy, ix) = sum_j m_j exp(-((U - u_j)^2 + V^2) / 2 sigma^2),   U = X cos az + Y sin az,  V = -X sin az + Y cos az,
      X = (ix - N / 2) qpixsize,  Y = (iy - N / 2) qpixsize,  ix along the axis of the x slopes,
  normalised to unit sum.  r_k = 0 gives the round beam.

Image of sub-aperture k (LgsModel), phase in microns:
  tile     a = mask exp(i (2 pi / lambda phase - halfxy)), pdiam x pdiam, as the Shack-Hartmann image forms it
  spot     I = |fft2(a zero-padded to N)|^2;  J = I circularly convolved with K_k
  binning  sums of J over the nrebin x nrebin blocks of the UNROLLED binmap (geom_init.py:751: the window is centred on
           pixel N / 2, where the kernel's centre sends the spot), times the Shack-Hartmann image's normalisation
           nphotons fluxPerSub_k / (sum of the window): `image`.  `hr_image` is J under the Parseval scale
           nphotons fluxPerSub_k / (N^2 sum mask^2): its sum over N x N is nphotons fluxPerSub_k, the kernel has unit sum.
  noise    the Shack-Hartmann pixel rule (csrc/aomarl_dev.h sh_noise, oracle aoref_sh_noise), idx = flat index of the cube
  slopes   centre of gravity, (sum v x / sum v - offset) scale in arcsec, all x then all y, minus the reference slopes

Second formulation (`form="lags"`, what the device computes): I is the DFT of the tile's autocorrelation
R(s) = sum_p a(p + s) conj(a(p)), |s| <= pdiam - 1 per axis, which does not wrap because 2 pdiam - 1 < N, so
  J(k) = sum_s R(s) Kt_k(s) exp(-2 pi i k . s / N),   Kt_k(s) = sum_j K_k(j) exp(+2 pi i j . s / N):
one pruned DFT over (2 pdiam - 1)^2 lags; R Kt is Hermitian, only the half sx >= 0 is kept ([2 pdiam - 1][pdiam] complex
per sub-aperture) and only the window's rows and columns are evaluated.

Cone (cone_trace_model): pupil-grid pixel (x, y) samples layer l at c_L + delta_l ((x, y) - c_p), delta_l = 1 - alt_l /
gsalt, c_p = (n - 1) / 2, c_L = c_p + (wxo, wyo) (the layer coordinate today's trace gives to c_p), bilinear with the
trace's edge rule.  Written as ((x, y) + (wxo, wyo)) + (delta_l - 1) ((x, y) - c_p), one fused multiply-add: delta = 1
is today's trace to the bit.

    python -m ao_marl_amd.lgs <config> [--llt x y] [--gsalt h]
        long-exposure Strehl of the NGS SH integrator, the LGS loop with centre launch and with side launch
"""
import ctypes as C
import os

import numpy as np

from . import libaomarl as la
from . import params as P
from .attachments import le_strehl
from .loop_sensor import LoopSensor
from .pyramid import pyr_noise

__all__ = ["lgs_kernels", "lgs_profile", "lgs_nphotons", "cone_deltas", "cone_trace_model", "LgsModel", "NativeLgs",
           "LgsSensor"]

FWHM2SIGMA = 2.35482005
ARCSEC_PER_RAD = 206265.     # the reference's constant (lgs_init.py:109)
LGS_SIZES = ((16, 64), (8, 32))      # (pdiam, N) the device kernel is built for (csrc/aomarl_lgs_host.h)


# ------------------------------------------------------------------------------------------------ profile, photons
def lgs_profile(profile="gauss1", mean_alt=90e3, fwhm=10e3):
    """(alt, prof): "gauss1" -- one Gaussian of `fwhm` metres about `mean_alt` on a grid of 100 m -- or a pair
    (alt, prof) with equally spaced altitudes, checked and returned as float64."""
    if isinstance(profile, str):
        if profile != "gauss1":
            raise ValueError("lgs profile %r: 'gauss1' or a pair (alt, prof); the reference's sodium files are its data "
                             "and are not shipped" % (profile,))
        if not (mean_alt > 0 and fwhm > 0):
            raise ValueError("lgs profile gauss1: mean altitude %r and FWHM %r must be positive" % (mean_alt, fwhm))
        alt = mean_alt + np.linspace(-2.5 * fwhm, 2.5 * fwhm, 501)
        return alt, np.exp(-(alt - mean_alt)**2 / (2 * (fwhm / FWHM2SIGMA)**2))
    try:
        alt, prof = profile
    except (TypeError, ValueError):
        raise ValueError("lgs profile: 'gauss1' or a pair (alt, prof)")
    alt, prof = np.asarray(alt, dtype=np.float64).reshape(-1), np.asarray(prof, dtype=np.float64).reshape(-1)
    if alt.size < 2 or alt.size != prof.size:
        raise ValueError("lgs profile: alt and prof must have the same length >= 2 (%d, %d)" % (alt.size, prof.size))
    # (a measured profile may dip below zero where the background was subtracted: accepted here, and lgs_kernels
    # drops the cells whose resampled mass is negative -- a kernel is a distribution of light)
    if not (np.all(np.isfinite(alt)) and np.all(np.isfinite(prof))) or not prof.sum() > 0:
        raise ValueError("lgs profile: prof must be finite with a positive sum")
    dh = np.diff(alt)
    if not np.all(dh > 0) or np.abs(dh - dh[0]).max() > 1e-6 * abs(dh[0]):
        raise ValueError("lgs profile: alt must be increasing and equally spaced")
    return alt, prof


def lgs_nphotons(p_wfs, p_tel, ittime, laserpower=0., lgsreturnperwatt=0.):
    """geom_init.py:391-392: lgsreturnperwatt laserpower optthroughput (D / nxsub)^2 1e4 ittime with a laser, otherwise
    the NGS rule (magnitude and zero point)."""
    sub = (p_tel.diam / p_wfs.nxsub)**2.
    if laserpower > 0:
        return float(lgsreturnperwatt * laserpower * p_wfs.optthroughput * sub * 1e4 * ittime)
    zerop = p_wfs.zerop if p_wfs.zerop != 0 else 1e11
    return float(zerop * 10.**(-0.4 * p_wfs.gsmag) * ittime * p_wfs.optthroughput * sub)


# ------------------------------------------------------------------------------------------------ the kernel
def lgs_kernels(sz, sh, p_tel, alt_na, prof_na, lltx, llty, beamsize):
    """K [nvalid][N][N] (float64, unit sum each) of the sub-apertures of the NGS geometry `sh` (geometry.sh_geometry's
    result: validsubsx, validsubsy, npix, nxsub) on the sizes `sz` (geometry.sh_sizes: Ntot, Nfft, qpixsize).  See the
    module's docstring for the rule."""
    N = int(sz.Ntot)
    if int(sz.Ntot) != int(sz.Nfft):
        raise NotImplementedError("lgs_kernels: Ntot = %d != Nfft = %d (the hrmap path) is not covered" % (sz.Ntot, sz.Nfft))
    if not beamsize > 0:
        raise ValueError("lgs_kernels: beamsize = %r arcsec must be positive" % (beamsize,))
    if not (np.isfinite(lltx) and np.isfinite(llty)):
        raise ValueError("lgs_kernels: the launch telescope's position (%r, %r) is not finite" % (lltx, llty))
    alt, prof = lgs_profile((alt_na, prof_na))
    npix, nx, q = int(sh.npix), int(sh.nxsub), float(sz.qpixsize)
    d = p_tel.diam / nx
    xsubs = np.linspace((d - p_tel.diam) / 2, (p_tel.diam - d) / 2, nx) if nx > 1 else np.zeros(1)
    x = xsubs[np.asarray(sh.validsubsx, dtype=np.int64) // npix]
    y = xsubs[np.asarray(sh.validsubsy, dtype=np.int64) // npix]
    r, az = np.hypot(x - lltx, y - llty), np.arctan2(y - llty, x - lltx)
    hG = float(np.sum(alt * prof) / np.sum(prof))
    if not hG > 0:
        raise ValueError("lgs_kernels: the profile's mean altitude %g m is not positive" % hG)
    sig = beamsize / FWHM2SIGMA
    profcum = np.concatenate([[0.], np.cumsum(prof)])
    cell = q / 2
    J = int(np.ceil(N * q / cell))                           # cells out to the window's diagonal and beyond
    uc = (np.arange(2 * J + 1) - J) * cell
    edges = np.concatenate([uc - cell / 2, [uc[-1] + cell / 2]])
    pix = (np.arange(N) - N / 2) * q
    X, Y = pix[None, :], pix[:, None]
    K = np.zeros((x.size, N, N))
    for k in range(x.size):
        zh = (alt - hG) * (ARCSEC_PER_RAD * r[k] / hG**2)
        if r[k] > 0 and zh[1] > zh[0]:
            he = np.concatenate([[zh[0]], 0.5 * (zh[1:] + zh[:-1]), [zh[-1]]])       # the reference's avg_zhc
            m = np.diff(np.interp(edges, he, profcum))
        else:
            m = np.zeros(uc.size)
            m[J] = profcum[-1]
        keep = np.nonzero(m > 0)[0]               # (cells of negative mass, a measured profile's background, are dropped)
        ca, sa = np.cos(az[k]), np.sin(az[k])
        U, V = X * ca + Y * sa, -X * sa + Y * ca
        line = np.zeros((N, N))
        for j in keep:
            line += m[j] * np.exp(-(U - uc[j])**2 / (2 * sig**2))
        Kk = line * np.exp(-V**2 / (2 * sig**2))
        K[k] = Kk / Kk.sum()
    return K


def impulse_kernels(nvalid, N):
    """K = delta at (N / 2, N / 2): the NGS image."""
    K = np.zeros((int(nvalid), int(N), int(N)))
    K[:, N // 2, N // 2] = 1.
    return K


# ------------------------------------------------------------------------------------------------ the cone
def cone_deltas(alts, gsalt):
    """delta_l = 1 - alt_l / gsalt; refuses a guide star at or below the highest layer."""
    alts = np.asarray(alts, dtype=np.float64).reshape(-1)
    if not gsalt > 0 or not np.isfinite(gsalt):
        raise ValueError("lgs: gsalt = %r m must be positive and finite" % (gsalt,))
    if alts.size and gsalt <= alts.max():
        raise ValueError("lgs: gsalt = %g m is not above the highest layer (%g m)" % (gsalt, alts.max()))
    return 1. - alts / float(gsalt)


def cone_trace_model(screens, atm_off, deltas, n, dtype=np.float64):
    """The atmosphere's phase [n][n] through the cone: sum over the layers, in order, of screen l [dim][dim] sampled at
    ((x, y) + atm_off[l]) + (delta_l - 1) ((x, y) - (n - 1) / 2), bilinear, zero outside, the last cell clamped (the
    oracle's aoref_raytrace).  float32: the arithmetic of the device's kernel, the position one fused multiply-add."""
    dt = np.dtype(dtype).type
    c = dt(0.5 * (n - 1))
    xs = np.arange(n).astype(dt)
    out = np.zeros((n, n), dtype=dt)
    for scr, (xo, yo), dl in zip(screens, atm_off, deltas):
        scr = np.asarray(scr, dtype=dt)
        dim = scr.shape[0]
        m = dt(np.float64(dl) - 1.0)

        def pos(off):
            base = xs + dt(off)
            if dt is np.float32:             # fma(m, x - c, x + off): one rounding
                return (base.astype(np.float64) + np.float64(m) * (xs - c).astype(np.float64)).astype(np.float32)
            return base + m * (xs - c)
        fx, fy = pos(xo), pos(yo)
        ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        wx, wy = (fx - ix.astype(dt)).astype(dt), (fy - iy.astype(dt)).astype(dt)
        okx, oky = (ix >= 0) & (ix < dim), (iy >= 0) & (iy < dim)
        ixc, iyc = np.clip(ix, 0, dim - 1), np.clip(iy, 0, dim - 1)
        ix1, iy1 = np.minimum(ixc + 1, dim - 1), np.minimum(iyc + 1, dim - 1)
        one = dt(1)
        top = (one - wx)[None, :] * scr[iyc][:, ixc] + wx[None, :] * scr[iyc][:, ix1]
        bot = (one - wx)[None, :] * scr[iy1][:, ixc] + wx[None, :] * scr[iy1][:, ix1]
        v = (one - wy)[:, None] * top + wy[:, None] * bot
        out = (out + np.where(oky[:, None] & okx[None, :], v, dt(0))).astype(dt)
    return out


# ------------------------------------------------------------------------------------------------ the model
class LgsModel(object):
    """The LGS image and slopes of the Shack-Hartmann system `s` (system.SimArrays: pupil, maps, photometry, centroid
    convention) with the kernels K [nvalid][N][N].  dtype: np.float64 (the definition) or np.float32 (the same
    statement in single precision, lag formulation: the yardstick of the device's error)."""

    def __init__(self, s, kernels, nphotons=None, noise=None, dtype=np.float64):
        self.s, self.dtype = s, np.dtype(dtype)
        self.ctype = np.complex128 if self.dtype == np.float64 else np.complex64
        self.n, self.pd, self.N, self.npix, self.nrebin, self.nvalid = (int(v) for v in (
            s.n, s.pdiam, s.nfft, s.npix, s.nrebin, s.nvalid))
        self.w = self.npix * self.nrebin
        if self.w > self.N:
            raise ValueError("lgs: the window npix nrebin = %d exceeds N = %d" % (self.w, self.N))
        if 2 * self.pd - 1 >= self.N:
            raise ValueError("lgs: 2 pdiam - 1 = %d lags wrap on N = %d" % (2 * self.pd - 1, self.N))
        self.indi = (self.N - self.w) // 2 + (1 if (self.w % 2 != self.N % 2) else 0)
        pm0 = np.asarray(s.phasemap, dtype=np.int64)[0]
        self.x0, self.y0 = pm0 % self.n, pm0 // self.n
        k = np.arange(self.pd)
        self.rows = self.y0[:, None, None] + k[None, :, None]
        self.cols = self.x0[:, None, None] + k[None, None, :]
        self.mask = np.asarray(s.mpupil, dtype=np.float64)[self.rows, self.cols]
        self.halfxy = np.asarray(s.halfxy, dtype=np.float64).reshape(self.pd, self.pd)
        self.flux = np.asarray(s.flux, dtype=np.float64)
        self.nphot = float(s.nphot if nphotons is None else nphotons)
        if not (self.nphot > 0 and np.isfinite(self.nphot)):
            raise ValueError("lgs: nphotons = %r must be positive and finite" % (self.nphot,))
        self.noise = float(s.noise if noise is None else noise)
        self.k2pi = 2 * np.pi / float(s.wfs_lambda)
        self.cog_offset, self.cog_scale = float(s.cog_offset), float(s.cog_scale)
        self.ref = np.zeros(2 * self.nvalid)
        self.set_kernels(kernels)

    def set_kernels(self, kernels):
        K = np.asarray(kernels, dtype=np.float64)
        if K.shape != (self.nvalid, self.N, self.N):
            raise ValueError("lgs kernels: shape %r, expected %r" % (K.shape, (self.nvalid, self.N, self.N)))
        if not np.all(np.isfinite(K)) or np.any(K < 0) or np.any(K.sum(axis=(1, 2)) <= 0):
            raise ValueError("lgs kernels: finite, not negative, each with a positive sum")
        # (the device holds the kernels in float32: a comparison with it hands the model the rounded numbers)
        self.K = K
        ft = np.fft.fft2(self.K)
        self.Kft = ft
        L = self.pd - 1
        sy = np.arange(-L, L + 1) % self.N
        self.Kt = np.conj(ft[:, sy][:, :, :self.pd])              # [nvalid][2 pd - 1][pd]: Kt(sy, sx >= 0)

    def set_ref(self, ref=None):
        self.ref = np.zeros(2 * self.nvalid) if ref is None else \
            np.asarray(ref, dtype=np.float64).reshape(2 * self.nvalid).copy()

    # ---- the tile
    def tiles(self, phase):
        dt = self.dtype
        ph = np.asarray(phase, dtype=dt)[self.rows, self.cols]
        ang = (dt.type(self.k2pi) * ph - self.halfxy.astype(dt)[None]).astype(dt)
        return (self.mask.astype(dt) * np.exp(1j * ang)).astype(self.ctype)

    # ---- formulation 1: transforms
    def _hr_fft(self, phase):
        a = self.tiles(phase)
        f = np.zeros((self.nvalid, self.N, self.N), dtype=self.ctype)
        f[:, :self.pd, :self.pd] = a
        F = np.fft.fft2(f).astype(self.ctype)
        I = (F.real**2 + F.imag**2).astype(self.dtype)
        J = np.fft.ifft2(np.fft.fft2(I).astype(self.ctype) * self.Kft.astype(self.ctype)).real
        return J.astype(self.dtype)

    # ---- formulation 2: lags
    def _hr_lags(self, phase, window=True):
        dt, ct, pd, N = self.dtype, self.ctype, self.pd, self.N
        a = self.tiles(phase)
        L = pd - 1
        ap = np.zeros((self.nvalid, pd + 2 * L, 2 * pd), dtype=ct)
        ap[:, L:L + pd, :pd] = a
        ac = np.conj(a)
        R = np.zeros((self.nvalid, 2 * L + 1, pd), dtype=ct)
        for sy in range(-L, L + 1):
            for sx in range(pd):
                R[:, sy + L, sx] = (ap[:, L + sy:L + sy + pd, sx:sx + pd] * ac).sum(axis=(1, 2), dtype=ct)
        Gm = (R * self.Kt.astype(ct)).astype(ct)
        kk = np.arange(self.indi, self.indi + self.w) if window else np.arange(N)
        sy = np.arange(-L, L + 1)
        Ey = np.exp(-2j * np.pi * ((kk[:, None] * sy[None, :]) % N) / N).astype(ct)            # [rows][2 pd - 1]
        cx = np.where(np.arange(pd) == 0, 1., 2.)
        Ex = (cx[:, None] * np.exp(-2j * np.pi * ((np.arange(pd)[:, None] * kk[None, :]) % N) / N)).astype(ct)
        T = np.matmul(Ey[None], Gm).astype(ct)                                                 # [nvalid][rows][pd]
        return np.matmul(T, Ex[None]).real.astype(dt)

    def hr_image(self, phase, form="fft"):
        """J [nvalid][N][N] of one phase [n][n] under the Parseval scale: each sums to nphotons fluxPerSub_k."""
        J = self._hr_fft(phase) if form == "fft" else self._hr_lags(phase, window=False)
        lit = (self.mask**2).sum(axis=(1, 2))
        sc = self.nphot * self.flux / (self.N**2 * np.maximum(lit, 1e-300))
        return J * sc.astype(self.dtype)[:, None, None]

    def image(self, phase, form=None):
        """bincube [nvalid][npix^2] of one phase [n][n] (microns), noise-free.  form: "fft" or "lags" (default: fft in
        float64, lags in float32)."""
        dt = self.dtype
        form = ("fft" if dt == np.float64 else "lags") if form is None else form
        i0, w = self.indi, self.w
        if form == "fft":
            win = self._hr_fft(phase)[:, i0:i0 + w, i0:i0 + w]
        elif form == "lags":
            win = self._hr_lags(phase, window=True)
        else:
            raise ValueError("lgs image: form %r ('fft' or 'lags')" % (form,))
        b = win.reshape(self.nvalid, self.npix, self.nrebin, self.npix, self.nrebin).sum(axis=(2, 4), dtype=dt)
        b = b.reshape(self.nvalid, self.npix * self.npix)
        tot = b.sum(axis=1, dtype=dt)
        g = np.where(tot > 0, dt.type(self.nphot) * self.flux.astype(dt) / np.where(tot > 0, tot, 1), 0).astype(dt)
        return (b * g[:, None]).astype(dt)

    def slopes(self, cube):
        dt, nv, npix = self.dtype, self.nvalid, self.npix
        im = np.asarray(cube, dtype=dt).reshape(nv, npix, npix)
        ax = np.arange(npix).astype(dt)
        tot = im.sum(axis=(1, 2), dtype=dt)
        sx = (im * ax[None, None, :]).sum(axis=(1, 2), dtype=dt)
        sy = (im * ax[None, :, None]).sum(axis=(1, 2), dtype=dt)
        ok = tot != 0
        safe = np.where(ok, tot, 1)
        off, sc = dt.type(self.cog_offset), dt.type(self.cog_scale)
        s = np.concatenate([np.where(ok, (sx / safe - off) * sc, 0), np.where(ok, (sy / safe - off) * sc, 0)]).astype(dt)
        return (s - self.ref.astype(dt)).astype(dt)

    def measure(self, phase, noise=False, seeds=None, frames=None, form=None):
        """phase [nenv][n][n] -> (cube [nenv][nvalid][npix^2], slopes [nenv][2 nvalid]).  noise: draw the model's noise
        with seeds[e] and frames[e]."""
        phase = np.asarray(phase)
        if phase.ndim == 2:
            phase = phase[None]
        cubes, sl = [], []
        for e in range(phase.shape[0]):
            b = self.image(phase[e], form)
            if noise and self.noise >= 0:
                b = pyr_noise(b.astype(np.float32), self.noise, seeds[e], frames[e]).astype(self.dtype)
            cubes.append(b)
            sl.append(self.slopes(b))
        return np.stack(cubes), np.stack(sl)


# ------------------------------------------------------------------------------------------------ the device object
def _check_size(s):
    if (int(s.pdiam), int(s.nfft)) not in LGS_SIZES:
        raise NotImplementedError("NativeLgs: pdiam = %d, N = %d: the kernel is built for %s" % (
            s.pdiam, s.nfft, ", ".join("pdiam = %d, N = %d" % t for t in LGS_SIZES)))


class NativeLgs(object):
    """aomarl_lgs_* for `nenv` environments of the Shack-Hartmann system `s`: the model on the GPU, fp32."""

    def __init__(self, s, nenv, kernels, nphotons=None, noise=None, device="cuda:0"):
        import torch
        if not torch.cuda.is_available():
            raise la.AomarlError("NativeLgs needs a GPU (the NumPy statement is LgsModel)")
        _check_size(s)
        self.lib, self.device, self.s, self.nenv = la.load(), torch.device(device), s, int(nenv)
        self.n, self.nvalid, self.npix, self.N = int(s.n), int(s.nvalid), int(s.npix), int(s.nfft)
        self.noise = float(s.noise if noise is None else noise)
        d = la.LgsDesc()
        d.nenv, d.n, d.pdiam, d.N, d.npix, d.nrebin, d.nvalid = (self.nenv, self.n, int(s.pdiam), self.N, self.npix,
                                                                 int(s.nrebin), self.nvalid)
        d.lambda_um, d.nphotons, d.noise = float(s.wfs_lambda), float(s.nphot if nphotons is None else nphotons), self.noise
        d.cog_offset, d.cog_scale = float(s.cog_offset), float(s.cog_scale)
        pm0 = np.asarray(s.phasemap, dtype=np.int64)[0]
        keep = [np.ascontiguousarray(s.mpupil, dtype=np.float32), np.ascontiguousarray(s.halfxy, dtype=np.float32),
                np.ascontiguousarray(s.flux, dtype=np.float32), np.ascontiguousarray(pm0 % self.n, dtype=np.int32),
                np.ascontiguousarray(pm0 // self.n, dtype=np.int32)]
        d.mpupil, d.halfxy, d.flux = (la.fptr(a) for a in keep[:3])
        d.sub_x0, d.sub_y0 = la.iptr(keep[3]), la.iptr(keep[4])
        self.ptr = C.c_void_p()
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_lgs_create(C.byref(d), C.byref(self.ptr)))
        f32 = dict(dtype=torch.float32, device=self.device)
        self.image = torch.zeros(self.nenv, self.nvalid, self.npix * self.npix, **f32)
        self.slopes = torch.zeros(self.nenv, 2 * self.nvalid, **f32)
        if kernels is not None:                 # (None: the impulse at (N / 2, N / 2), what create starts with)
            self.set_kernels(kernels)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.aomarl_lgs_destroy(self.ptr)
            self.ptr = None

    def set_kernels(self, kernels):
        K = np.ascontiguousarray(kernels, dtype=np.float32)
        if K.shape != (self.nvalid, self.N, self.N):
            raise ValueError("lgs kernels: shape %r, expected %r" % (K.shape, (self.nvalid, self.N, self.N)))
        la.check(self.lib.aomarl_lgs_set_kernels(self.ptr, la.fptr(K)))

    def set_ref(self, ref=None):
        r = None if ref is None else np.ascontiguousarray(ref, dtype=np.float32).reshape(2 * self.nvalid)
        la.check(self.lib.aomarl_lgs_set_ref(self.ptr, None if r is None else la.fptr(r)))

    def trace(self, sim, deltas, atm=True, dms=True, env_begin=0, env_count=None):
        """The cone trace of a HipSim's state into its sensor phase buffer (k_lgs_trace)."""
        n = self.nenv - env_begin if env_count is None else int(env_count)
        dl = np.ascontiguousarray(np.asarray(deltas, dtype=np.float64) - 1.0, dtype=np.float32)
        sim._need_phase()
        sim._ensure_shape()
        fl = (la.TRACE_ATMOS if atm else 0) | (la.TRACE_DMS if dms else 0) | la.TRACE_RESET
        la.check(self.lib.aomarl_lgs_trace(self.ptr, sim.ctx, C.byref(sim.st), la.fptr(dl), int(dl.size), int(env_begin), n,
                                           fl, la.raw_stream(self.device)))

    def measure(self, phase, noise=False, seeds=None, frame=None, env_begin=0, env_count=None, write_cube=True):
        """phase: float32 device tensor [nenv][n][n]; writes self.slopes (and self.image with write_cube) rows of the
        environments measured.  noise: seeds, frame: the simulator's int32 device tensors [nenv]; frame advances by one."""
        n = self.nenv - env_begin if env_count is None else int(env_count)
        if tuple(phase.shape) != (self.nenv, self.n, self.n) or str(phase.dtype) != "torch.float32" or \
                not phase.is_cuda or not phase.is_contiguous():
            raise ValueError("phase must be a contiguous float32 device tensor [%d][%d][%d]" % (self.nenv, self.n, self.n))
        if noise and (seeds is None or frame is None or seeds.numel() != self.nenv or frame.numel() != self.nenv):
            raise ValueError("noise needs the seeds and frame counters of all %d environments" % self.nenv)
        fl = (la.LGS_NOISE if noise else 0) | (la.LGS_WRITE_CUBE if write_cube else 0)
        la.check(self.lib.aomarl_lgs_measure(self.ptr, phase.data_ptr(), int(env_begin), n, fl,
                                             seeds.data_ptr() if noise else None, frame.data_ptr() if noise else None,
                                             self.image.data_ptr(), self.slopes.data_ptr(), la.raw_stream(self.device)))
        return self.slopes


class _ModelBackend(object):
    """LgsModel behind NativeLgs's interface: the CPU path of an LgsSensor (device="cpu"), NumPy arrays."""

    def __init__(self, s, nenv, kernels, nphotons=None, noise=None):
        self.model = LgsModel(s, kernels, nphotons=nphotons, noise=noise)
        self.device, self.nenv, self.noise, self.s = "cpu", int(nenv), self.model.noise, s
        self.image = np.zeros((self.nenv, self.model.nvalid, self.model.npix**2))
        self.slopes = np.zeros((self.nenv, 2 * self.model.nvalid))

    def set_kernels(self, kernels):
        self.model.set_kernels(kernels)

    def set_ref(self, ref=None):
        self.model.set_ref(ref)

    def trace(self, sim, deltas, atm=True, dms=True, env_begin=0, env_count=None):
        """cone_trace_model (float32, the device kernel's arithmetic) on the screens of a CPU simulator that keeps one
        oracle per environment (`sim.sims`: screens, wfs_phase, raytrace_wfs), the mirrors on top as it traces them"""
        sims = getattr(sim, "sims", None)
        if sims is None:
            raise NotImplementedError("the cone trace on the CPU needs a simulator with one oracle per environment "
                                      "(`sims`); cone_trace_model is the NumPy statement")
        n = self.nenv - env_begin if env_count is None else int(env_count)
        for o in sims[env_begin:env_begin + n]:
            if atm:
                o.wfs_phase[:] = cone_trace_model(o.screens, self.s.wfs_atm_off, deltas, self.s.n, dtype=np.float32)
            else:
                o.wfs_phase[:] = 0
            if dms:
                o.raytrace_wfs(atm=False, dms=True, reset=False)

    def measure(self, phase, noise=False, seeds=None, frame=None, env_begin=0, env_count=None, write_cube=True):
        n = self.nenv - env_begin if env_count is None else int(env_count)
        phase = np.asarray(phase, dtype=np.float64).reshape(self.nenv, self.model.n, self.model.n)
        sl = slice(env_begin, env_begin + n)
        self.image[sl], self.slopes[sl] = self.model.measure(
                phase[sl], noise, None if seeds is None else np.asarray(seeds)[sl],
                None if frame is None else np.asarray(frame)[sl])
        if noise and frame is not None and self.noise >= 0:
            frame[sl] += 1
        return self.slopes


# ------------------------------------------------------------------------------------------------ the sensor
class LgsSensor(LoopSensor):
    """A laser guide star on the guide star of a VecRlSupervisor's NGS Shack-Hartmann system.

        lgs = LgsSensor(sup, gsalt=90e3, llt=(0., 0.))
        cmat = lgs.calibrate()            # flat reference, Btt modes pushed through the mirrors, command matrix
        lgs.start()                       # the supervisor's loop now runs on the LGS
        ... sup.next_part_one(); sup.next_part_two(...) or VecAoEnv.step (the call-by-call path) ...
        lgs.stop()

    Values default to attributes of p_wfss[0] where it has them.  kernels: K [nvalid][N][N] in place of the elongation
    kernel (lgs.impulse_kernels: the NGS spots through the cone)."""
    slot = "lgs"

    def __init__(self, sup, gsalt=None, llt=None, beamsize=None, profile=None, laserpower=None, lgsreturnperwatt=None,
                 noise=None, kernels=None):
        ps, like = sup.config, sup.config.p_wfss[0]

        def pick(v, names, default):
            if v is not None:
                return v
            for nm in names:
                got = getattr(like, nm, None)
                if got:
                    return got
            return default
        gsalt = float(pick(gsalt, ("gsalt",), 90e3))
        if llt is None:
            llt = (float(getattr(like, "lltx", 0.) or 0.), float(getattr(like, "llty", 0.) or 0.))
        self.lltx, self.llty = float(llt[0]), float(llt[1])
        self.beamsize = float(pick(beamsize, ("beamsize",), 0.8))
        self.laserpower = float(pick(laserpower, ("laserpower",), 0.))
        self.lgsreturnperwatt = float(pick(lgsreturnperwatt, ("lgsreturnperwatt",), 0.))
        profile = pick(profile, ("proftype",), "gauss1")
        sysm, s = sup.sysm, sup.s
        self.sup, self.gsalt, self.s = sup, gsalt, s
        self.deltas = cone_deltas(sysm.atm.alt, gsalt)
        for d in s.dms:
            if float(d.alt) != 0.:
                raise NotImplementedError("LgsSensor: a mirror conjugated to %g m is seen through the cone; only mirrors "
                                          "in the pupil (alt = 0) are covered" % d.alt)
        w = sysm.wfss[0]
        self.alt_na, self.prof_na = lgs_profile(profile)
        self.kernels = lgs_kernels(w, w, ps.p_tel, self.alt_na, self.prof_na, self.lltx, self.llty, self.beamsize) \
            if kernels is None else np.asarray(kernels, dtype=np.float64)
        self.nphotons = lgs_nphotons(like, ps.p_tel, ps.p_loop.ittime, self.laserpower, self.lgsreturnperwatt)
        self.nenv, self.nvalid, self.nslope = int(sup.sim.nenv), int(s.nvalid), 2 * int(s.nvalid)
        nz = float(s.noise if noise is None else noise)
        if str(sup.sim.device) == "cpu":
            self.native = _ModelBackend(s, self.nenv, self.kernels, self.nphotons, nz)
        else:
            self.native = NativeLgs(s, self.nenv, self.kernels, self.nphotons, nz, device=sup.sim.device)
        self.device = self.native.device
        self.cmat, self.ref, self.linearity, self._cmat_dev, self._attached = None, None, None, None, False

    # ---- measurements
    def trace(self, atm=True, dms=True, env_begin=0, env_count=None):
        """The sensor's pupil phase of the simulator's state through the cone, into the simulator's phase buffer."""
        self.native.trace(self.sup.sim, self.deltas, atm, dms, env_begin, env_count)

    def measure(self, phase=None, noise=None, env_begin=0, env_count=None, write_cube=True):
        """Slopes [nenv][2 nvalid] of `phase` (default: the simulator's sensor phase buffer, as `trace` left it).
        noise (default: whenever the sensor has noise): with the simulator's seeds and frame counters."""
        sim = self.sup.sim
        if phase is None:
            phase = sim.t["wfs_phase"]
        noisy = (self.native.noise >= 0) if noise is None else bool(noise)
        if noisy and self.device == "cpu":
            raise NotImplementedError("measure: noise uses the device simulator's seeds and frame counters")
        return self.native.measure(phase, noisy, sim.t["seeds"] if noisy else None, sim.t["frame"] if noisy else None,
                                   env_begin, env_count, write_cube)

    def set_kernels(self, kernels):
        if self._attached:
            raise RuntimeError("set_kernels: stop() first")
        self.native.set_kernels(kernels)
        self.kernels = np.asarray(kernels, dtype=np.float64)
        self.cmat, self._cmat_dev = None, None

    # ---- what LoopSensor asks for (in the calibration the mirrors are in the pupil: the cone does not touch them)
    keeps_phase = True                          # the buffer holds the phase the sensor just saw through the cone

    def _pupil(self):
        return np.asarray(self.s.mpupil).reshape(-1) != 0

    def _quiet(self):
        self.measure(noise=False, write_cube=False)

    def _trace(self):
        self.trace()

    def _measure(self):
        self.measure(write_cube=False)

    def calibrate(self, push_um=0.01):
        if not push_um > 0:
            raise ValueError("calibrate: push_um = %r must be positive" % (push_um,))
        return LoopSensor.calibrate(self, push_um)

    # ---- the loop
    def start(self):
        if self.device == "cpu" and getattr(self.sup.sim, "sims", None) is None:
            raise NotImplementedError("LgsSensor.start: the loop on the CPU needs a simulator with one oracle per environment")
        return LoopSensor.start(self)

    def control(self):
        if self.device != "cpu":
            return LoopSensor.control(self)
        # one oracle per environment: its err and com, as aoref_ls_control leaves them
        cm = np.ascontiguousarray(self.cmat, dtype=np.float32)
        for o, sl in zip(self.sup.sim.sims, np.ascontiguousarray(self.native.slopes, dtype=np.float32)):
            o.L.aoref_ls_control(cm, cm.shape[0], cm.shape[1], sl, float(self.sup.gain), o.err, o.com)


# ------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    import argparse
    from .env import VecRlSupervisor
    ap = argparse.ArgumentParser(prog="python -m ao_marl_amd.lgs",
                                 description="Long-exposure Strehl of the NGS SH integrator, of the LGS loop with centre "
                                             "launch and of the LGS loop with side launch, on the same seeds")
    ap.add_argument("config", nargs="?", default="production_sh_10x10_2m",
                    help="a built-in configuration or a parameter file (.py)")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--llt", type=float, nargs=2, default=None, metavar=("X", "Y"),
                    help="the side launch position in metres (default: one telescope diameter off along x)")
    ap.add_argument("--gsalt", type=float, default=90e3)
    ap.add_argument("--beamsize", type=float, default=0.8)
    ap.add_argument("--nfilt", type=int, default=5, help="Btt modes filtered from the command matrices")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    ps = P.load_param_file(a.config) if a.config.endswith(".py") and os.path.exists(a.config) else P.builtin(a.config)
    sup = VecRlSupervisor(ps, dict(n_reverse_filtered_from_cmat=a.nfilt), a.envs, device=a.device)
    side = tuple(a.llt) if a.llt is not None else (float(ps.p_tel.diam), 0.)
    print("config %s, %d environments, %d frames, gain %g, %d modes filtered, gsalt %g m" % (
        ps.simul_name, a.envs, a.frames, sup.gain, a.nfilt, a.gsalt))
    print("long-exposure Strehl  NGS SH integrator %.4f" % le_strehl(sup, a.frames))
    for name, llt in (("centre launch", (0., 0.)), ("side launch (%g, %g) m" % side, side)):
        lgs = LgsSensor(sup, gsalt=a.gsalt, llt=llt, beamsize=a.beamsize)
        lgs.calibrate()
        lgs.start()
        sr = le_strehl(sup, a.frames)
        lgs.stop()
        print("long-exposure Strehl  LGS loop, %-28s %.4f   (doubled-push deviation %.3g)" % (name, sr, lgs.linearity))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
