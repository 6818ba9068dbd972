"""Shared by tests/test_lgs.py and tests/test_gpu_lgs.py: the 10x10 system the LGS tests run on, the fixture written from
the reference's own make_lgs_prof1d (tests/golden/lgs.npz, tools/gen_golden_lgs.py), and the phases the tests look at."""
import os

import numpy as np

from ao_marl_amd import geometry as G
from ao_marl_amd import lgs as L
from ao_marl_amd import params as P
from ao_marl_amd import system

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lgs.npz")
CONFIG = "production_sh_10x10_2m"
_CACHE = {}


def golden():
    if "z" not in _CACHE:
        with np.load(GOLDEN) as z:
            _CACHE["z"] = {k: z[k] for k in z.files}
    return _CACHE["z"]


def params(alts=None, pupdiam=None):
    """The 10x10 parameters; alts: the layers' altitudes in place of the file's (as many layers as the list is long,
    equal fractions, the first layer's wind); pupdiam: the pupil's diameter in pixels in place of the derived one (80:
    sub-apertures of 8 pixels on N = 32)."""
    ps = P.builtin(CONFIG)
    if pupdiam is not None:
        ps.p_geom.pupdiam = int(pupdiam)
    if alts is not None:
        a, k = ps.p_atmos, len(alts)
        first = lambda v: np.asarray(v).reshape(-1)[0]  # noqa: E731
        a.nscreens, a.alt, a.frac = k, np.asarray(alts, dtype=np.float64), np.full(k, 1.0 / k)
        a.windspeed = np.full(k, float(first(a.windspeed)))
        a.winddir = np.full(k, float(first(a.winddir)))
        a.L0 = np.full(k, float(first(a.L0)))
    return ps


def system_of(alts=None, pupdiam=None):
    """(ParamSet, geometry.build_system result, SimArrays), built once per variant; read only."""
    key = ("sys", None if alts is None else tuple(alts), pupdiam)
    if key not in _CACHE:
        ps = params(alts, pupdiam)
        sysm = G.build_system(ps)
        _CACHE[key] = (ps, sysm, system.from_system(sysm, strehl_halfwin=8))
    return _CACHE[key]


def kernels(llt, profile="gauss1", beamsize=0.8, pupdiam=None):
    """lgs_kernels of the 10x10 system for a launch position, built once; read only."""
    key = ("K", tuple(llt), profile if isinstance(profile, str) else id(profile), beamsize, pupdiam)
    if key not in _CACHE:
        ps, sysm, _ = system_of(pupdiam=pupdiam)
        alt, prof = L.lgs_profile(profile)
        _CACHE[key] = L.lgs_kernels(sysm.wfss[0], sysm.wfss[0], ps.p_tel, alt, prof, llt[0], llt[1], beamsize)
    return _CACHE[key]


def moments(a):
    """(sigma_major, sigma_minor, angle) of the second-moment matrix of a[i0][i1], as tools/gen_golden_lgs.py records
    them: the major axis' angle atan2(along i0, along i1) folded into (-pi/2, pi/2]; and the centroid (c0, c1)."""
    a = np.asarray(a, dtype=np.float64)
    i0, i1 = np.indices(a.shape)
    s = a.sum()
    c0, c1 = (a * i0).sum() / s, (a * i1).sum() / s
    m00, m11 = (a * (i0 - c0)**2).sum() / s, (a * (i1 - c1)**2).sum() / s
    m01 = (a * (i0 - c0) * (i1 - c1)).sum() / s
    w, v = np.linalg.eigh(np.array([[m11, m01], [m01, m00]]))
    ang = np.arctan2(v[1, 1], v[0, 1])
    ang = ang - np.pi if ang > np.pi / 2 else (ang + np.pi if ang <= -np.pi / 2 else ang)
    return np.sqrt(w[1]), np.sqrt(w[0]), ang, c0, c1


def tilt_phase(s, arcsec, axis):
    """A tilt of `arcsec` on the sky: phase [n][n] in microns, along x (axis 1) or y (axis 0)."""
    ps = system_of()[0]
    um_per_pixel = arcsec / G.RAD2ARCSEC * (ps.p_tel.diam / s.pupdiam) * 1e6
    r = (np.arange(s.n) - (s.n - 1) / 2.) * um_per_pixel
    return np.tile(r[None, :], (s.n, 1)) if axis == 1 else np.tile(r[:, None], (1, s.n))


def smooth_phases(s, nenv, seed, rms_um=0.15, waves_of_tilt=0.0):
    """`nenv` random smooth phases [n][n] in microns (low-pass filtered white noise, `rms_um` rms); the last one carries
    `waves_of_tilt` wavelengths of tilt per sub-aperture along x on top (the spot near the window's edge)."""
    rng = np.random.default_rng(seed)
    n = s.n
    f = np.fft.fftfreq(n)[:, None]**2 + np.fft.fftfreq(n)[None, :]**2
    filt = np.exp(-f / (2 * (2.0 / s.pupdiam * 3)**2))
    out = []
    for e in range(nenv):
        p = np.fft.ifft2(np.fft.fft2(rng.normal(size=(n, n))) * filt).real
        p = p - p.mean()
        out.append(p * (rms_um / p.std()))
    if waves_of_tilt:
        out[-1] = out[-1] + (np.arange(n) - n / 2.)[None, :] * (waves_of_tilt * s.wfs_lambda / s.pdiam)
    return np.stack(out)
