#!/usr/bin/env python3
"""Generate the laser-guide-star kernel fixture by IMPORTING the reference's pure-Python init code.

Runs ONLY in the build container (needs the reference tree, see tools/_ref_shims.py); what it writes,
tests/golden/lgs.npz, is plain data.  The reference's own `init_wfs_geom` (through `tel_init`) and `make_lgs_prof1d`
(shesha/init/lgs_init.py) run unmodified on production_sh_10x10_2m with gsalt = 90 km, the launch telescope at
lltx = llty = -3 m (where make_lgs_prof1d's exchange of validsubsx / validsubsy in its off-axis distance is harmless),
a beam of 0.8 arcsec, and the mean of the reference's sodium profiles.  Recorded: the profile and its altitudes,
_azimuth, _beam, _qpixsize, Ntot, validsubs, for every sub-aperture the second moments of the reference's
_lgskern[:, :, k] (eigen-sigmas in pixels and the major axis' angle, the array's first index taken as x), and four
whole kernels as stored.

Usage: python tools/gen_golden_lgs.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shims  # noqa: E402
import gen_golden  # noqa: E402

import numpy as np  # noqa: E402

GSALT, LLT, BEAM = 90e3, -3.0, 0.8
WHOLE = (0, 7, 31, 63)


def moments(a):
    """(sigma_major, sigma_minor, angle) of the second-moment matrix of the image a[i0][i1]; the angle is that of the
    major axis, atan2(component along i0, component along i1), folded into (-pi/2, pi/2]."""
    a = np.asarray(a, dtype=np.float64)
    i0, i1 = np.indices(a.shape)
    s = a.sum()
    c0, c1 = (a * i0).sum() / s, (a * i1).sum() / s
    m00 = (a * (i0 - c0)**2).sum() / s
    m11 = (a * (i1 - c1)**2).sum() / s
    m01 = (a * (i0 - c0) * (i1 - c1)).sum() / s
    w, v = np.linalg.eigh(np.array([[m11, m01], [m01, m00]]))
    ang = np.arctan2(v[1, 1], v[0, 1])
    if ang > np.pi / 2:
        ang -= np.pi
    if ang <= -np.pi / 2:
        ang += np.pi
    return np.sqrt(w[1]), np.sqrt(w[0]), ang


def main():
    gen_golden.install_fake_native()
    _ref_shims.install()
    from shesha.util.utilities import load_config_from_file
    from shesha.init.geom_init import tel_init
    from shesha.init.lgs_init import make_lgs_prof1d
    import carmaWrap
    cfg = load_config_from_file(os.path.join(_ref_shims.REF, "data/par/par4rl/production", "production_sh_10x10_2m.py"))
    w = cfg.p_wfss[0]
    w.set_gsalt(GSALT)
    w.set_lltx(LLT)
    w.set_llty(LLT)
    w.set_beamsize(BEAM)
    ctx = carmaWrap.context.get_instance_1gpu(0)
    tel_init(ctx, cfg.p_geom, cfg.p_tel, cfg.p_atmos.r0, cfg.p_loop.ittime, cfg.p_wfss)
    prof = np.load(os.path.join(_ref_shims.REF, "data", "allProfileNa_withAltitude.npy"))
    alt, na = prof[0, :].astype(np.float64), np.mean(prof[1:, :], axis=0).astype(np.float64)
    make_lgs_prof1d(w, cfg.p_tel, na, alt, w.beamsize, center="image")
    kern = np.asarray(w._lgskern)                       # [Ntot][Ntot][nvalid]
    # the reference hands its arrays to a column-major library: the first index of _lgskern[:, :, k] is x
    mom = np.array([moments(kern[:, :, k].T) for k in range(kern.shape[2])])
    out = dict(alt=alt, prof=na, azimuth=np.asarray(w._azimuth, dtype=np.float64), beam=np.asarray(w._beam, dtype=np.float32),
               qpixsize=np.array(float(w._qpixsize)), Ntot=np.array(int(w._Ntot)), Nfft=np.array(int(w._Nfft)),
               nrebin=np.array(int(w._nrebin)), npix=np.array(int(w.npix)), pdiam=np.array(int(w._pdiam)),
               validsubsx=np.asarray(w._validsubsx, dtype=np.int32), validsubsy=np.asarray(w._validsubsy, dtype=np.int32),
               gsalt=np.array(GSALT), lltx=np.array(LLT), llty=np.array(LLT), beamsize=np.array(BEAM),
               sigma_major=mom[:, 0], sigma_minor=mom[:, 1], angle=mom[:, 2],
               whole_index=np.array(WHOLE, dtype=np.int32),
               whole=np.stack([kern[:, :, k] for k in WHOLE]).astype(np.float32))
    path = os.path.join(os.path.dirname(HERE), "tests", "golden", "lgs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "size: %.1f KB" % (os.path.getsize(path) / 1e3))
    print("Ntot %d  nvalid %d  qpixsize %.6f  sigma_minor %.4f .. %.4f  sigma_major %.4f .. %.4f" % (
        out["Ntot"], kern.shape[2], out["qpixsize"], mom[:, 1].min(), mom[:, 1].max(), mom[:, 0].min(), mom[:, 0].max()))


if __name__ == "__main__":
    main()
