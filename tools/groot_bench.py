"""Times the GROOT covariance model (ao_marl_amd.groot) of the 40x40 system on the device against its NumPy statement:
cerr for one atmosphere and for a sweep of 16, calias (npts = 3), and k_groot_form alone (device events).

    python tools/groot_bench.py [--params production_sh_40x40_8m_3layers] [--reps 5] [--no-cpu]

The source is a mapping built from the calibrated system (no loop is run: the model needs none).  The CPU statement is
float64 NumPy on however many threads NumPy's BLAS takes; --no-cpu skips it (a 40x40 cerr takes it about a minute)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def source_of(sup):
    """the keys GrootModel reads, from a supervisor (what VecRoket.to_dict writes, without histories)"""
    from ao_marl_amd import modal
    cal, s, ps, dm = sup.cal, sup.s, sup.config, sup.s.dms[0]
    a, w = ps.p_atmos, ps.p_wfss[0]
    frac = np.asarray(a.frac, dtype=np.float64)
    IF = cal.IF.tocsc()[:, :-2].T.tocsr().astype(np.float32)
    return {"P": np.asarray(cal.P), "Btt": np.asarray(cal.Btt), "R": np.asarray(s.cmat, dtype=np.float32),
            "IF.data": IF.data, "IF.indices": IF.indices, "IF.indptr": IF.indptr,
            "TT": np.asarray(cal.IF.tocsc()[:, -2:].todense(), dtype=np.float32), "tar_lambda": np.asarray([s.tar_lambda]),
            "spup": np.asarray(s.spupil, dtype=np.float32),
            "Nact": modal.nact_geom(dm.i1, dm.j1, dm.pitch, ps.p_dms[s.dm_index[0]].coupling, dm.n2 - dm.n1 + 1),
            "dm.xpos": dm.xpos, "dm.ypos": dm.ypos, "_Param_atmos__r0": float(a.r0), "_Param_atmos__alt": np.asarray(a.alt),
            "_Param_atmos__L0": np.asarray(a.L0), "_Param_atmos__windspeed": np.asarray(a.windspeed),
            "_Param_atmos__winddir": np.asarray(a.winddir), "_Param_atmos__frac": frac / frac.sum(),
            "_Param_atmos__nscreens": int(a.nscreens), "_Param_loop__ittime": float(ps.p_loop.ittime),
            "_Param_controller__gain": float(sup.gain), "_Param_wfs__xpos": np.asarray([w.xpos]),
            "_Param_wfs__ypos": np.asarray([w.ypos]), "_Param_wfs__Lambda": np.asarray([w.Lambda]),
            "_Param_wfs__nxsub": np.asarray([w.nxsub]), "_Param_wfs__npix": np.asarray([w.npix]),
            "_Param_tel__diam": float(ps.p_tel.diam), "_Param_tel__cobs": float(ps.p_tel.cobs),
            "_Param_geom__pupdiam": int(sup.sysm.geom.pupdiam), "_Param_dm__nact": np.asarray([d.nact for d in ps.p_dms]),
            "_Param_dm__unitpervolt": np.asarray([d.unitpervolt for d in ps.p_dms], dtype=np.float64),
            "_Param_wfs___validsubsx": np.asarray(s.validsubsx), "_Param_wfs___validsubsy": np.asarray(s.validsubsy)}


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--params", default="production_sh_40x40_8m_3layers")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args(argv)
    from ao_marl_amd import groot
    from ao_marl_amd.env import VecAoEnv
    env = VecAoEnv(a.params, 1, geo=True, frame_pipeline=False)
    src = source_of(env.supervisor)
    g = groot.GrootModel(src, device=str(env.supervisor.device), batch_max=16)
    print("%s: %d actuators, %d modes, %d sub-apertures, %d layers" % (a.params, g.na, g.nm, g.nsub, g.nl))
    sweep = dict(speed=np.linspace(0.5, 2.0, 16)[:, None] * g.speed[None, :], r0=np.linspace(0.08, 0.2, 16))
    rows = [("cerr modal, 1 atmosphere", lambda m: m.cerr()), ("cerr modal, sweep of 16", lambda m: m.cerr(**sweep)),
            ("calias modal, npts 3", lambda m: m.calias())]
    for name, fn in rows:
        print("device  %-28s %9.2f ms" % (name, 1e3 * timed(lambda: fn(g), a.reps)))
    # the form kernel alone (its tap copy included), by device events around the second of two calls
    import torch

    def form_ms(spec, which, out):
        g._form_native(spec, which, out, 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g._form_native(spec, which, out, 0)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for B, over in ((1, {}), (16, sweep)):
        ms = form_ms(g.cerr_spec(**over)[0], "act", g._zeros(B, g.na))
        n = B * g.na * g.na * 3 * g.nl
        print("device  k_groot_form, Cerr, B = %-3d %9.3f ms   %.1f M evaluations, %.2f G evaluations / s" %
              (B, ms, n / 1e6, n / ms / 1e6))
    ms = form_ms(g.calias_specs(3)[0], "sub", g._zeros(1, 2 * g.nsub))
    n = g.nsub * g.nsub * 15
    print("device  k_groot_form, Calias XX     %9.3f ms   %.1f M evaluations, %.2f G evaluations / s" % (ms, n / 1e6, n / ms / 1e6))
    torch.cuda.synchronize()
    if not a.no_cpu:
        c = groot.GrootModel(src, device="cpu")
        for name, fn in (rows[0], rows[2]):
            t = time.perf_counter()
            ref = fn(c)
            dt = time.perf_counter() - t
            got = fn(g)
            print("NumPy   %-28s %9.2f ms   device against it: %.2e of the largest value" %
                  (name, 1e3 * dt, np.abs(got - ref).max() / np.abs(ref).max()))


if __name__ == "__main__":
    main()
