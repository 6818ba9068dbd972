"""Pyramid wavefront sensor ("pyrhr": four pupil images, circular or user-given modulation, field stop).

Three layers:
  PyramidModel    the definition of the sensor, NumPy, float64 (or float32 for error estimates); the CPU path
  NativePyramid   aomarl_pyr_* (csrc/aomarl_pyr.hip): the same model on the GPU in fp32
  PyramidSensor   a sensor on the guide star of a VecRlSupervisor's system: calibration (`calibrate`) and the closed
                  loop (`start` / `stop`: the supervisor's next_part_one then measures with the pyramid and integrates
                  err = -cmat_pyr . slopes_pyr)

The geometry is geometry.pyr_sizes / pyr_geometry (the reference's init_wfs_size, pyramid branch, and
init_pyrhr_geom).  The image formation itself is not in the reference tree (it lives in the external library); the
model below is this project's statement of it, and the choices the reference's Python does not pin are listed in
DESIGN.md ("Pyramid sensor", unpinned).

Model, per environment, phase phi [n][n] in microns, y the slow axis and x the fast one:
  field    f_k = mpupil exp(i (2 pi / lambda phi + cx_k (x - n/2) + cy_k (y - n/2))), placed in an Nfft^2 zero array at
           rows and columns Nfft/2 - n/2 .. Nfft/2 + n/2 - 1 (where init_pyrhr_geom places `pup`)
  images   F_k = fft2(f_k) exp(i halfxy) submask;  hr = sum_k w_k |ifft2(F_k)|^2, k in index order
  filter   pixel_filter: hr = Re ifft2(fft2(hr) sincar)
  binning  binimg = sums of hr over nrebin x nrebin blocks, times nphotons / (sum_k w_k  sum mpupil^2): an open field
           stop passes nphotons in all (Parseval), what a stop cuts is lost
  noise    noise < 0: none; 0: Poisson; > 0: Poisson + N(0, noise): one Philox block per (pixel, frame), the words and
           thresholds of the Shack-Hartmann pixels (csrc/aomarl_dev.h sh_noise), idx = flat pixel index of binimg
  slopes   per valid point i the pixels q0..q3 of the four validsubs blocks (at row-,col- / row+,col+ / row+,col- /
           row-,col+ of the image centre), I_i = sum q;
           raw x = ((q1 + q3) - (q0 + q2)) / norm, raw y = ((q1 + q2) - (q0 + q3)) / norm,
           norm = mean_i I_i (methods 0, 1) or I_i (methods 2, 3); norm < thresh (or norm == 0): slope 0;
           methods 1, 3: s_scale sin(pi / 2 raw), methods 0, 2: s_scale raw; all x, then all y; minus the reference
           slopes (set_ref).

    python -m ao_marl_amd.pyramid <config>      long-exposure Strehl of the SH and of the pyramid integrator
"""
import ctypes as C
import os

import numpy as np

from . import geometry as G
from . import libaomarl as la
from . import params as P
from .attachments import le_strehl
from .loop_sensor import LoopSensor

__all__ = ["PyramidModel", "NativePyramid", "PyramidSensor", "pyr_noise"]


# ------------------------------------------------------------------------------------------------ noise (NumPy)
def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def _u01(x):
    return ((x >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def pyr_noise(img, sigma, seed, frame):
    """The draw rule of a detector pixel (csrc/aomarl_dev.h sh_noise, oracle aoref_sh_noise) on a float32 image: pixel
    idx (flat) of frame `frame` owns the Philox block {idx, frame, 0, 4} under the key {seed, "AOMR"}."""
    lam = np.asarray(img, dtype=np.float32).reshape(-1)
    if sigma < 0:
        return lam.reshape(np.shape(img)).copy()
    idx = np.arange(lam.size, dtype=np.uint64)
    z = np.zeros_like(idx)
    x0, x1, x2, _ = _philox4x32_10(idx, z + np.uint64(int(frame) & 0xFFFFFFFF), z, z + np.uint64(4),
                                   int(seed) & 0xFFFFFFFF, 0x414F4D52)
    u = _u01(x0)
    r = np.sqrt(np.float32(-2.0) * np.log(_u01(x1))).astype(np.float32)
    a = np.float32(6.28318530717958647692) * _u01(x2)
    zn = r * np.cos(a).astype(np.float32)
    # Poisson: inversion below 30, rounded normal above
    small = (lam > 0) & (lam < 30)
    p = np.exp(-np.where(small, lam, 0)).astype(np.float32)
    c = p.copy()
    k = np.zeros(lam.size, dtype=np.int32)
    live = small & (u > c)
    while live.any() and int(k.max()) < 200:
        k = np.where(live, k + 1, k)
        p = np.where(live, p * (lam / np.maximum(k, 1).astype(np.float32)), p).astype(np.float32)
        cn = (c + p).astype(np.float32)
        stop = cn == c
        c = np.where(live, cn, c)
        live = live & ~stop & (u > c) & (k < 200)
    big = np.floor(lam + np.sqrt(np.maximum(lam, 0)) * zn + np.float32(0.5))
    v = np.where(small, k.astype(np.float32), np.where(lam > 0, np.maximum(big, 0), 0)).astype(np.float32)
    if sigma > 0:
        v = v + np.float32(sigma) * (r * np.sin(a).astype(np.float32))
    return v.astype(np.float32).reshape(np.shape(img))


# ------------------------------------------------------------------------------------------------ the model
class PyramidModel(object):
    """The sensor of a geometry.pyr_geometry Bag `pg` (see the module's docstring).  dtype: np.float64 (the
    definition) or np.float32 (the same statement in single precision: the yardstick of the device's error)."""

    def __init__(self, pg, method=1, thresh=1.0e-4, pixel_filter=True, noise=None, dtype=np.float64):
        if method not in (0, 1, 2, 3):
            raise ValueError("pyramid centroider method %r: 0..3" % (method,))
        self.pg, self.method, self.thresh, self.pixel_filter = pg, int(method), float(thresh), bool(pixel_filter)
        self.noise = float(pg.noise if noise is None else noise)
        self.dtype = np.dtype(dtype)
        self.ctype = np.complex128 if self.dtype == np.float64 else np.complex64
        self.N, self.n, self.nrebin, self.nvalid = int(pg.Nfft), int(pg.n), int(pg.nrebin), int(pg.nvalid)
        self.nb = self.N // self.nrebin
        self.mpupil = np.asarray(pg.mpupil, dtype=self.dtype)
        self.lit = float(np.sum(np.asarray(pg.mpupil, dtype=np.float64)**2))
        self.mask = (np.asarray(pg.submask, dtype=self.dtype) *
                     np.exp(1j * np.asarray(pg.halfxy, dtype=self.dtype))).astype(self.ctype)
        self.sincar = np.asarray(pg.sincar, dtype=self.dtype)
        self.vx, self.vy = np.asarray(pg.validsubsx, dtype=np.int64), np.asarray(pg.validsubsy, dtype=np.int64)
        self.ref = np.zeros(2 * self.nvalid, dtype=np.float64)
        self.s_scale = float(pg.s_scale)
        self.set_modulation(pg.pyr_cx, pg.pyr_cy, None)

    def set_modulation(self, cx, cy, weights=None, s_scale=None):
        cx, cy = np.asarray(cx, dtype=np.float64).reshape(-1), np.asarray(cy, dtype=np.float64).reshape(-1)
        w = np.ones(cx.size) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        _check_modulation(cx, cy, w)
        # (the device holds the points in float32: the model takes the same numbers)
        self.cx, self.cy, self.w = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (cx, cy, w))
        if s_scale is not None:
            self.s_scale = float(s_scale)

    def set_ref(self, ref=None):
        self.ref = np.zeros(2 * self.nvalid) if ref is None else np.asarray(ref, dtype=np.float64).reshape(2 * self.nvalid).copy()

    def image(self, phase):
        """binimg [nb][nb] of one phase [n][n] (microns), noise-free."""
        dt, N, n = self.dtype, self.N, self.n
        phase = np.asarray(phase, dtype=dt)
        k2pi = dt.type(2 * np.pi / self.pg.Lambda)
        xs = (np.arange(n) - n // 2).astype(dt)
        o = N // 2 - n // 2
        hr = np.zeros((N, N), dtype=dt)
        for k in range(self.cx.size):
            arg = k2pi * phase + (dt.type(self.cx[k]) * xs[None, :] + dt.type(self.cy[k]) * xs[:, None])
            f = np.zeros((N, N), dtype=self.ctype)
            f[o:o + n, o:o + n] = self.mpupil * np.exp(1j * arg.astype(dt)).astype(self.ctype)
            Fk = np.fft.fft2(f).astype(self.ctype) * self.mask
            z = np.fft.ifft2(Fk).astype(self.ctype)
            hr += dt.type(self.w[k]) * (z.real**2 + z.imag**2)
        if self.pixel_filter:
            hr = np.fft.ifft2(np.fft.fft2(hr.astype(self.ctype)).astype(self.ctype) * self.sincar).real.astype(dt)
        b = hr.reshape(self.nb, self.nrebin, self.nb, self.nrebin).sum(axis=(1, 3), dtype=dt)
        return b * dt.type(self.pg.nphotons / (float(np.sum(self.w)) * self.lit))

    def slopes(self, binimg, method=None):
        dt = self.dtype
        method = self.method if method is None else int(method)
        nv = self.nvalid
        q = np.asarray(binimg, dtype=dt)[self.vx, self.vy].reshape(4, nv)
        tot = q.sum(axis=0)
        norm = tot if method >= 2 else np.full(nv, tot.mean(), dtype=dt)
        ok = ~(norm < self.thresh) & (norm != 0)
        safe = np.where(ok, norm, 1)
        sx = np.where(ok, ((q[1] + q[3]) - (q[0] + q[2])) / safe, 0)
        sy = np.where(ok, ((q[1] + q[2]) - (q[0] + q[3])) / safe, 0)
        s = np.concatenate([sx, sy]).astype(dt)
        if method & 1:
            s = np.sin(dt.type(np.pi / 2) * s)
        s = np.where(np.concatenate([ok, ok]), dt.type(self.s_scale) * s, 0)
        return (s - self.ref.astype(dt)).astype(dt)

    def measure(self, phase, noise=False, seeds=None, frames=None, method=None):
        """phase [nenv][n][n] -> (binimg [nenv][nb][nb], slopes [nenv][2 nvalid]).  noise: draw the model's noise with
        seeds[e] and frames[e]."""
        phase = np.asarray(phase)
        if phase.ndim == 2:
            phase = phase[None]
        imgs, sl = [], []
        for e in range(phase.shape[0]):
            b = self.image(phase[e])
            if noise and self.noise >= 0:
                b = pyr_noise(b.astype(np.float32), self.noise, seeds[e], frames[e]).astype(self.dtype)
            imgs.append(b)
            sl.append(self.slopes(b, method))
        return np.stack(imgs), np.stack(sl)


def _check_modulation(cx, cy, w):
    if cx.size < 1 or cy.size != cx.size or w.size != cx.size:
        raise ValueError("set_modulation: cx, cy and weights must have the same, positive number of points "
                         "(%d, %d, %d)" % (cx.size, cy.size, w.size))
    if not (np.all(np.isfinite(cx)) and np.all(np.isfinite(cy))):
        raise ValueError("set_modulation: a modulation point is not finite")
    if not np.all(np.isfinite(w)) or np.any(w < 0) or not np.sum(w) > 0:
        raise ValueError("set_modulation: weights must be finite, not negative, with a positive sum")


# ------------------------------------------------------------------------------------------------ the device object
class NativePyramid(object):
    """aomarl_pyr_* for `nenv` environments: the model on the GPU, fp32."""

    def __init__(self, pg, nenv, npts_max=None, thresh=1.0e-4, pixel_filter=True, noise=None, device="cuda:0",
                 batch_kib=0):
        import torch
        if not torch.cuda.is_available():
            raise la.AomarlError("NativePyramid needs a GPU (the NumPy statement is PyramidModel)")
        self.lib, self.device, self.pg, self.nenv = la.load(), torch.device(device), pg, int(nenv)
        self.nb, self.nvalid, self.n = int(pg.Nfft) // int(pg.nrebin), int(pg.nvalid), int(pg.n)
        self.noise = float(pg.noise if noise is None else noise)
        npts = int(np.size(pg.pyr_cx))
        d = la.PyrDesc()
        d.nenv, d.n, d.Nfft, d.nrebin, d.nvalid = self.nenv, self.n, int(pg.Nfft), int(pg.nrebin), self.nvalid
        d.npts_max, d.pixel_filter, d.batch_kib = int(npts_max or max(npts, 1)), int(bool(pixel_filter)), int(batch_kib)
        d.lambda_um, d.nphotons, d.noise, d.thresh = float(pg.Lambda), float(pg.nphotons), self.noise, float(thresh)
        keep = [np.ascontiguousarray(getattr(pg, k), dtype=np.float32) for k in ("mpupil", "halfxy", "submask", "sincar")]
        keep += [np.ascontiguousarray(getattr(pg, k), dtype=np.int32) for k in ("validsubsx", "validsubsy")]
        d.mpupil, d.halfxy, d.submask, d.sincar = (la.fptr(a) for a in keep[:4])
        d.validsubsx, d.validsubsy = la.iptr(keep[4]), la.iptr(keep[5])
        self.ptr = C.c_void_p()
        with torch.cuda.device(self.device):
            la.check(self.lib.aomarl_pyr_create(C.byref(d), C.byref(self.ptr)))
        f32 = dict(dtype=torch.float32, device=self.device)
        self.image = torch.zeros(self.nenv, self.nb, self.nb, **f32)
        self.slopes = torch.zeros(self.nenv, 2 * self.nvalid, **f32)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.aomarl_pyr_destroy(self.ptr)
            self.ptr = None

    def set_modulation(self, cx, cy, weights, s_scale):
        cx, cy, w = (np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (cx, cy, weights))
        la.check(self.lib.aomarl_pyr_set_modulation(self.ptr, la.fptr(cx), la.fptr(cy), la.fptr(w), int(cx.size),
                                                    float(s_scale)))

    def set_ref(self, ref=None):
        r = None if ref is None else np.ascontiguousarray(ref, dtype=np.float32).reshape(2 * self.nvalid)
        la.check(self.lib.aomarl_pyr_set_ref(self.ptr, None if r is None else la.fptr(r)))

    def measure(self, phase, method=1, noise=False, seeds=None, frame=None, env_begin=0, env_count=None):
        """phase: float32 device tensor [nenv][n][n]; writes self.image / self.slopes rows of the environments measured.
        noise: seeds, frame: int32 / uint32 device tensors [nenv] (the simulator's); frame advances by one."""
        n = self.nenv - env_begin if env_count is None else int(env_count)
        if tuple(phase.shape) != (self.nenv, self.n, self.n) or str(phase.dtype) != "torch.float32" or \
                not phase.is_cuda or not phase.is_contiguous():
            raise ValueError("phase must be a contiguous float32 device tensor [%d][%d][%d]" % (self.nenv, self.n, self.n))
        fl = la.PYR_NOISE if noise else 0
        if noise and (seeds is None or frame is None or seeds.numel() != self.nenv or frame.numel() != self.nenv):
            raise ValueError("noise needs the seeds and frame counters of all %d environments" % self.nenv)
        la.check(self.lib.aomarl_pyr_measure(self.ptr, phase.data_ptr(), int(env_begin), n, fl, int(method),
                                             seeds.data_ptr() if noise else None, frame.data_ptr() if noise else None,
                                             self.image.data_ptr(), self.slopes.data_ptr(), la.raw_stream(self.device)))
        return self.slopes


class _ModelBackend(object):
    """PyramidModel behind NativePyramid's interface: the CPU path of a PyramidSensor (device="cpu"), NumPy arrays."""

    def __init__(self, pg, nenv, thresh=1.0e-4, pixel_filter=True, noise=None):
        self.model = PyramidModel(pg, thresh=thresh, pixel_filter=pixel_filter, noise=noise)
        self.device, self.nenv, self.noise = "cpu", int(nenv), self.model.noise
        self.image = np.zeros((self.nenv, self.model.nb, self.model.nb))
        self.slopes = np.zeros((self.nenv, 2 * self.model.nvalid))

    def set_modulation(self, cx, cy, weights, s_scale):
        self.model.set_modulation(cx, cy, weights, s_scale)

    def set_ref(self, ref=None):
        self.model.set_ref(ref)

    def measure(self, phase, method=1, noise=False, seeds=None, frame=None, env_begin=0, env_count=None):
        n = self.nenv - env_begin if env_count is None else int(env_count)
        phase = np.asarray(phase, dtype=np.float64).reshape(self.nenv, self.model.n, self.model.n)
        sl = slice(env_begin, env_begin + n)
        self.image[sl], self.slopes[sl] = self.model.measure(
                phase[sl], noise, None if seeds is None else np.asarray(seeds)[sl],
                None if frame is None else np.asarray(frame)[sl], method)
        if noise and frame is not None and self.noise >= 0:
            frame[sl] += 1
        return self.slopes


# ------------------------------------------------------------------------------------------------ the sensor
def _pyr_params(nxsub, pyr_ampl, pyr_npts, fssize, fstop, Lambda, gsmag, noise, like):
    """A Param_wfs of type pyrhr with the photometry of the SH sensor `like`."""
    return P.Param_wfs(type="pyrhr", nxsub=int(nxsub), pyr_ampl=float(pyr_ampl), pyr_npts=int(pyr_npts),
                       fssize=float(fssize), fstop=fstop, Lambda=float(Lambda), gsmag=float(gsmag), noise=float(noise),
                       optthroughput=like.optthroughput, zerop=like.zerop if like.zerop != 0 else 1e11,
                       fracsub=like.fracsub, atmos_seen=1, xpos=like.xpos, ypos=like.ypos)


class PyramidSensor(LoopSensor):
    """A pyramid on the guide star of a VecRlSupervisor's system.

        pyr = PyramidSensor(sup, nxsub=20)
        cmat = pyr.calibrate()            # Btt modes pushed through the mirrors, flat reference, command matrix
        pyr.start()                       # the supervisor's loop now runs on the pyramid
        ... sup.next_part_one(); sup.next_part_two(...) or VecAoEnv.step (the call-by-call path) ...
        pyr.stop()

    PyramidSensor.from_geometry(...) builds one without a supervisor (measure(phase) only)."""
    slot = "pyramid"

    def __init__(self, sup, nxsub=None, pyr_ampl=3, pyr_npts=16, fssize=None, fstop="round", Lambda=None, gsmag=None,
                 noise=-1, method=1, thresh=1.0e-4, pixel_filter=True):
        ps, like = sup.config, sup.config.p_wfss[0]
        if nxsub is None:
            # twice the Shack-Hartmann's count where the pupil allows it: at the same count the pyramid's points (whole
            # pixels inside the pupil) give fewer slopes than the mirrors have modes, and the loop does not close
            pd = sup.sysm.geom.pupdiam
            nxsub = 2 * like.nxsub if pd % (2 * like.nxsub) == 0 else like.nxsub
        Lambda = like.Lambda if Lambda is None else Lambda
        if fssize is None:              # the reference's advice (geom_init.py:199): radius lambda / D . nxsub / 2
            fssize = nxsub * Lambda * 1e-6 / ps.p_tel.diam * G.RAD2ARCSEC
        p_wfs = _pyr_params(nxsub, pyr_ampl, pyr_npts, fssize, fstop, Lambda, like.gsmag if gsmag is None else gsmag,
                            noise, like)
        p_cen = P.Param_centroider(type="pyr", method=method, thresh=thresh)
        self._init(sup.sysm.geom, ps.p_tel, p_wfs, p_cen, ps.p_loop.ittime, sup.sim.device, sup.sim.nenv, pixel_filter)
        self.sup = sup

    @classmethod
    def from_geometry(cls, geom, p_tel, p_wfs, p_centroider=None, ittime=0.002, device="cuda:0", nenv=1,
                      pixel_filter=True):
        self = cls.__new__(cls)
        self._init(geom, p_tel, p_wfs, p_centroider or P.Param_centroider(type="pyr"), ittime, device, nenv, pixel_filter)
        self.sup = None
        return self

    def _init(self, geom, p_tel, p_wfs, p_cen, ittime, device, nenv, pixel_filter):
        self.p_wfs, self.p_tel = p_wfs, p_tel
        self.sizes = G.pyr_sizes(p_wfs, p_tel, geom.pupdiam)
        self.pg = G.pyr_geometry(p_wfs, self.sizes, geom, p_tel, ittime)
        if p_wfs.pyr_pos is None and int(p_wfs.pyr_npts) < 1:
            raise ValueError("pyramid: pyr_npts = %r modulation points" % (p_wfs.pyr_npts,))
        self.method, self.thresh = int(p_cen.method), float(p_cen.thresh)
        if self.method not in (0, 1, 2, 3):
            raise ValueError("pyramid centroider method %r: 0..3" % (p_cen.method,))
        self.nenv, self.nvalid, self.nslope = int(nenv), self.pg.nvalid, 2 * self.pg.nvalid
        if str(device) == "cpu":                # the model itself (float64, NumPy in and out)
            self.native = _ModelBackend(self.pg, nenv, thresh=self.thresh, pixel_filter=pixel_filter)
        else:
            self.native = NativePyramid(self.pg, nenv, thresh=self.thresh, pixel_filter=pixel_filter, device=device)
        self.device = self.native.device
        self.cx, self.cy = np.asarray(self.pg.pyr_cx, dtype=np.float64), np.asarray(self.pg.pyr_cy, dtype=np.float64)
        self.weights, self.s_scale = np.ones(self.cx.size), float(self.pg.s_scale)
        self.native.set_modulation(self.cx, self.cy, self.weights, self.s_scale)
        self.cmat, self.ref, self.linearity, self._cmat_dev, self._attached = None, None, None, None, False

    # ---- modulation
    def set_modulation(self, cx, cy, weights=None):
        """Modulation points in radians of phase per pupil pixel (pyr_geometry's pyr_cx / pyr_cy) and their weights."""
        cx, cy = np.asarray(cx, dtype=np.float64).reshape(-1), np.asarray(cy, dtype=np.float64).reshape(-1)
        w = np.ones(cx.size) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        _check_modulation(cx, cy, w)
        self.native.set_modulation(cx, cy, w, self.s_scale)
        self.cx, self.cy, self.weights = cx, cy, w

    def set_modulation_ampli(self, ampl):
        """wfsCompass.set_pyr_modulation_ampli: a circle of `ampl` lambda / D in the same number of points; the
        slopes' scale follows (rtc_init.py:221-222).  Returns the scale."""
        if not float(ampl) >= 0:
            raise ValueError("set_modulation_ampli: %r lambda / D" % (ampl,))
        w = P.Param_wfs(**{k: getattr(self.p_wfs, k) for k in P.Param_wfs._defaults})
        w.pyr_ampl, w.pyr_pos = float(ampl), None
        if int(w.pyr_npts) < 1:
            w.pyr_npts = self.cx.size
        cx, cy, _ = G.pyr_modulation(w, self.sizes, self.p_tel)
        scale = (w.Lambda * 1e-6 / self.p_tel.diam) * max(float(ampl), 1e-30) * G.RAD2ARCSEC
        self.native.set_modulation(cx, cy, np.ones(cx.size), scale)
        self.p_wfs, self.cx, self.cy, self.weights, self.s_scale = w, cx, cy, np.ones(cx.size), scale
        return scale

    # ---- measurements
    def measure(self, phase=None, noise=None, env_begin=0, env_count=None):
        """Slopes [nenv][2 nvalid] (device) of `phase` (default: the simulator's sensor phase, as raytrace_wfs left
        it).  noise (default: whenever the sensor has noise and a simulator whose counters it can use)."""
        sim = self.sup.sim if self.sup is not None else None
        if phase is None:
            if sim is None:
                raise ValueError("measure: a stand-alone sensor needs the phase")
            phase = sim.t["wfs_phase"]
        noisy = (self.native.noise >= 0 and sim is not None) if noise is None else bool(noise)
        if noisy and sim is None:
            raise ValueError("measure: noise needs a simulator's seeds and frame counters")
        return self.native.measure(phase, self.method, noisy, sim.t["seeds"] if noisy else None,
                                   sim.t["frame"] if noisy else None, env_begin, env_count)

    # ---- what LoopSensor asks for (the calibration pushes `push_um` small against the modulation radius: pyr_ampl
    # lambda / D of tilt is pyr_ampl lambda / 4 rms)
    def _pupil(self):
        return np.asarray(self.pg.mpupil).reshape(-1) != 0

    def _quiet(self):
        self.measure(noise=False)

    def _trace(self):
        self.sup.sim.raytrace_wfs(atm=True, dms=True, reset=True)

    def _measure(self):
        self.measure()


# ------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    import argparse
    from .env import VecRlSupervisor
    ap = argparse.ArgumentParser(prog="python -m ao_marl_amd.pyramid",
                                 description="Long-exposure Strehl of the SH integrator and of the pyramid integrator "
                                             "on the same seeds")
    ap.add_argument("config", nargs="?", default="production_sh_10x10_2m",
                    help="a built-in configuration or a parameter file (.py)")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--nxsub", type=int, default=None, help="points across the pupil (default: twice the SH's)")
    ap.add_argument("--ampl", type=float, default=3.0, help="modulation radius in lambda / D")
    ap.add_argument("--npts", type=int, default=16)
    ap.add_argument("--nfilt", type=int, default=5, help="Btt modes filtered from both command matrices")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    ps = P.load_param_file(a.config) if a.config.endswith(".py") and os.path.exists(a.config) else P.builtin(a.config)
    sup = VecRlSupervisor(ps, dict(n_reverse_filtered_from_cmat=a.nfilt), a.envs, device=a.device)
    sr_sh = le_strehl(sup, a.frames)
    pyr = PyramidSensor(sup, nxsub=a.nxsub, pyr_ampl=a.ampl, pyr_npts=a.npts)
    pyr.calibrate()
    pyr.start()
    sr_pyr = le_strehl(sup, a.frames)
    pyr.stop()
    print("config %s, %d environments, %d frames, gain %g, %d modes filtered" % (ps.simul_name, a.envs, a.frames, sup.gain,
                                                                                a.nfilt))
    print("pyramid: nxsub %d, Nfft %d, nrebin %d, %d valid points, %d modulation points of %g lambda/D, "
          "doubled-push deviation %.3g" % (pyr.pg.nxsub, pyr.pg.Nfft, pyr.pg.nrebin, pyr.nvalid, pyr.cx.size, a.ampl,
                                           pyr.linearity))
    print("long-exposure Strehl  SH integrator %.4f   pyramid integrator %.4f" % (sr_sh, sr_pyr))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
