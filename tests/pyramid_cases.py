"""Shared by tests/test_pyramid.py and tests/test_gpu_pyramid.py: the pyramid geometries of tests/golden/pyr_geom.npz
(written by tools/gen_golden_pyr.py from the reference's own init_wfs_size / init_pyrhr_geom) rebuilt with the project's
derivation, and the phases the tests look at."""
import hashlib
import os

import numpy as np

from ao_marl_amd import geometry as G
from ao_marl_amd import params as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyr_geom.npz")
TAGS = ("tinyA", "tinyB", "s10_10", "s10_20")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scalar(z, tag, k):
    return z["%s_s_%s" % (tag, k)].item()


def params_of(z, tag, **over):
    """(p_tel, p_wfs, ittime) of a fixture case; `over` replaces sensor parameters."""
    s = lambda k: scalar(z, tag, k)  # noqa: E731
    tel = P.Param_tel(diam=s("diam"), cobs=s("cobs"))
    kw = dict(type="pyrhr", nxsub=int(s("nxsub")), fssize=s("fssize"), fstop=str(z[tag + "_fstop"]),
              pyr_ampl=s("pyr_ampl"), pyr_npts=int(s("pyr_npts")), Lambda=s("Lambda"), gsmag=s("gsmag"),
              optthroughput=s("optthroughput"), zerop=s("zerop"), fracsub=s("fracsub"), noise=-1.)
    kw.update(over)
    return tel, P.Param_wfs(**kw), s("ittime")


def build(z, tag, **over):
    """(pupil geometry, sizes, pyramid geometry, p_tel, p_wfs) of a fixture case."""
    tel, w, ittime = params_of(z, tag, **over)
    geom = G.pupil_geometry(int(scalar(z, tag, "pupdiam")), tel)
    sz = G.pyr_sizes(w, tel, geom.pupdiam)
    return geom, sz, G.pyr_geometry(w, sz, geom, tel, ittime), tel, w


def lam_over_d(pg, tel):
    """lambda / D in arcsec"""
    return pg.Lambda * 1e-6 / tel.diam * G.RAD2ARCSEC


def tilt_phase(pg, tel, geom, amp, axis):
    """A tilt of `amp` lambda / D: amp * lambda microns across the pupil's diameter, along x (axis 1) or y (axis 0)."""
    r = (np.arange(pg.n) - pg.n / 2.) * (amp * pg.Lambda / geom.pupdiam)
    return np.tile(r[None, :], (pg.n, 1)) if axis == 1 else np.tile(r[:, None], (1, pg.n))


def smooth_phases(pg, tel, geom, nenv, seed, rms_um=0.15):
    """`nenv` random smooth phases [n][n] in microns (low-pass filtered white noise, `rms_um` rms), the last one with
    a 2 lambda / D tilt along x on top."""
    rng = np.random.default_rng(seed)
    n = pg.n
    f = np.fft.fftfreq(n)[:, None]**2 + np.fft.fftfreq(n)[None, :]**2
    filt = np.exp(-f / (2 * (2.0 / geom.pupdiam * 3)**2))        # features down to a sixth of the pupil
    out = []
    for e in range(nenv):
        p = np.fft.ifft2(np.fft.fft2(rng.normal(size=(n, n))) * filt).real
        p = p - p.mean()
        out.append(p * (rms_um / p.std()))
    out[-1] = out[-1] + tilt_phase(pg, tel, geom, 2.0, 1)
    return np.stack(out)
