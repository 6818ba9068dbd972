#!/usr/bin/env python3
"""Generate the pyramid-sensor geometry fixture by IMPORTING the reference's pure-Python init code.

Runs ONLY in the build container (needs the reference tree, see tools/_ref_shims.py); what it writes,
tests/golden/pyr_geom.npz, is plain data.  The reference's own `init_wfs_geom` (-> `init_wfs_size`, pyramid branch,
-> `init_pyrhr_geom`, shesha/init/geom_init.py) runs unmodified on an already initialised pupil geometry -- the
"not the first sensor" path -- for
  tinyA    pupdiam 32, nxsub 8,  no obstruction,   round stop    (whole arrays)
  tinyB    pupdiam 48, nxsub 12, obstruction 0.3,  square stop   (whole arrays)
  s10_10   the 10x10 / 2 m system's pupil, nxsub 10              (scalars, validsubs, cx / cy, SHA-256 of the planes)
  s10_20   the same, nxsub 20

Usage: python tools/gen_golden_pyr.py
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shims  # noqa: E402
import gen_golden  # noqa: E402

import numpy as np  # noqa: E402

ITTIME = 0.002


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pyr_wfs(conf, nxsub, fssize, fstop, npts=16, ampl=3.0):
    w = conf.Param_wfs()
    w.set_type("pyrhr")
    w.set_nxsub(nxsub)
    w.set_fssize(fssize)
    w.set_fstop(fstop)
    w.set_pyr_ampl(ampl)
    w.set_pyr_npts(npts)
    w.set_Lambda(0.5)
    w.set_gsmag(4.)
    w.set_optthroughput(0.12)
    w.set_zerop(1.e11)
    w.set_fracsub(0.8)
    w.set_atmos_seen(1)
    return w


def record(out, tag, w, g, p_tel, full):
    scal = dict(pupdiam=g.pupdiam, n=g._n, diam=p_tel.diam, cobs=p_tel.cobs, nxsub=w.nxsub, fssize=w.fssize,
                pdiam=w._pdiam, Nfft=w._Nfft, nrebin=w._nrebin, qpixsize=w._qpixsize, pixsize=w.pixsize,
                nvalid=w._nvalid, nphotons=w._nphotons, pyr_scale_pos=w._pyr_scale_pos, pyr_ampl=w.pyr_ampl,
                pyr_npts=w.pyr_npts, Lambda=w.Lambda, gsmag=w.gsmag, optthroughput=w.optthroughput, zerop=w.zerop,
                fracsub=w.fracsub, ittime=ITTIME,
                s_scale=(w.Lambda * 1e-6 / p_tel.diam) * w.pyr_ampl * (3600. * 360. / (2 * np.pi)))
    for k, v in scal.items():
        out["%s_s_%s" % (tag, k)] = np.array(v)
    out[tag + "_fstop"] = np.array(str(w.fstop))
    planes = dict(submask=np.asarray(w._submask, dtype=np.float32), halfxy=np.asarray(w._halfxy, dtype=np.float32),
                  sincar=np.asarray(w._sincar, dtype=np.float32), isvalid=np.asarray(w._isvalid, dtype=np.int32),
                  mpupil=np.asarray(g._mpupil, dtype=np.float32))
    for k, v in planes.items():
        out["%s_sha_%s" % (tag, k)] = np.array(sha(v))
        if full or v.size <= 4096:
            out["%s_%s" % (tag, k)] = v
    for k in ("_validsubsx", "_validsubsy", "_pyr_cx", "_pyr_cy"):
        out[tag + k] = np.asarray(getattr(w, k))


def tiny(conf, pupdiam, nxsub, cobs, fstop, fssize):
    from shesha.init.geom_init import geom_init, init_wfs_geom
    p_tel = conf.Param_tel()
    p_tel.set_diam(2.0)
    p_tel.set_cobs(cobs)
    g = conf.Param_geom()
    g.set_pupdiam(pupdiam)
    geom_init(g, p_tel)
    w = pyr_wfs(conf, nxsub, fssize, fstop)
    init_wfs_geom(w, 0.16, p_tel, g, ITTIME, verbose=0)
    return w, g, p_tel


def main():
    gen_golden.install_fake_native()
    _ref_shims.install()
    import shesha.config as conf
    from shesha.util.utilities import load_config_from_file
    from shesha.init.geom_init import tel_init, init_wfs_geom
    import carmaWrap
    out = {}
    w, g, t = tiny(conf, 32, 8, 0.0, "round", 1.0)
    record(out, "tinyA", w, g, t, True)
    w, g, t = tiny(conf, 48, 12, 0.3, "square", 1.2)
    record(out, "tinyB", w, g, t, True)
    cfg = load_config_from_file(os.path.join(_ref_shims.REF, "data/par/par4rl/production", "production_sh_10x10_2m.py"))
    ctx = carmaWrap.context.get_instance_1gpu(0)
    tel_init(ctx, cfg.p_geom, cfg.p_tel, cfg.p_atmos.r0, cfg.p_loop.ittime, cfg.p_wfss)
    for nxsub in (10, 20):
        w = pyr_wfs(conf, nxsub, 1.6, "round")
        init_wfs_geom(w, cfg.p_atmos.r0, cfg.p_tel, cfg.p_geom, ITTIME, verbose=0)
        record(out, "s10_%d" % nxsub, w, cfg.p_geom, cfg.p_tel, False)
    path = os.path.join(os.path.dirname(HERE), "tests", "golden", "pyr_geom.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "keys:", len(out), "size: %.1f KB" % (os.path.getsize(path) / 1e3))
    for k in sorted(out):
        if "_s_" in k:
            print(k, out[k])


if __name__ == "__main__":
    main()
