"""Times laser tomography (ao_marl_amd.tomography, csrc/aomarl_tomo.hip) on the device:

    python tools/tomo_bench.py [--reps 20] [--rounds 5] [--no-large]

  40x40 / 8 m, three layers, 256 environments        10x10 / 2 m, 64 environments        K = 4 stars at 90 km, 20 arcsec

Per shape, ms per call:
  trace              k_tomo_trace: the K planes of every environment
  trace + measure    ... then one aomarl_lgs_measure over the K nenv pseudo-environments (noise off, centre launch)
  control            LaserTomography.control(): est = R S, err = -cmat_tomo S + G voltage, com += gain err (matrices of
                     the sensor's shapes filled with small random numbers: the time does not depend on them)
  covariance         k_tomo_cov: C_SS [2 nvalid K]^2 in double, what calibrate() forms (one call per round)
Device events around `reps` calls, `rounds` times: the median and the spread (min .. max) of the rounds.  No threshold:
the figures go into DESIGN.md."""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.lgs_bench import timed  # noqa: E402


def run(name, nenv, reps, rounds, K=4, radius=20., field=25.):
    import torch
    from ao_marl_amd import geometry as G, lgs as L, params as P, system, tomography as T
    from ao_marl_amd.sim import HipSim
    ps = T.with_field(P.builtin(name), field)
    sysm = G.build_system(ps)
    s = system.from_system(sysm)
    sim = HipSim(s, nenv=nenv, keep_phase=True)
    sim.reset(np.arange(nenv) + 1234)
    stars = T.ring(K, radius)
    off, dm1, _ = T.constellation_offsets(sysm, stars)
    w = sysm.wfss[0]
    alt, prof = L.lgs_profile("gauss1")
    kern = L.lgs_kernels(w, w, ps.p_tel, alt, prof, 0., 0., 0.8)
    nat, tomo = L.NativeLgs(s, nenv * K, kern, noise=-1.), T.NativeTomo()
    planes = torch.zeros(nenv, K, s.n, s.n, dtype=torch.float32, device="cuda:0")
    ns, na = 2 * s.nvalid, s.nactu
    # the sensor's control() on buffers of its shapes (no calibration: R of a 40x40 system is minutes of host algebra)
    sen = T.LaserTomography.__new__(T.LaserTomography)
    sen.sup, sen.tomo, sen.polc = types.SimpleNamespace(sim=sim, gain=0.5), tomo, True
    sen.native, sen.nenv, sen.K, sen.nslope = nat, nenv, K, ns
    sen.est = torch.zeros(nenv, ns, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(1)
    rnd = lambda *sh: 1e-3 * torch.randn(*sh, device="cuda:0", generator=g)  # noqa: E731
    sen._dev = [rnd(na, K * ns), rnd(ns, K * ns), rnd(na, int(sim._frame_buf("voltage").shape[1]))]
    px, py = T.subap_centres(s, sysm.atm.pupixsize)
    lay = T.atmos_layers(sysm.atm.alt, ps.p_atmos.r0, ps.p_atmos.frac, ps.p_atmos.L0)

    def trace():
        tomo.trace(sim, off, dm1, planes)

    def both():
        tomo.trace(sim, off, dm1, planes)
        nat.measure(planes.reshape(nenv * K, s.n, s.n), write_cube=False)

    def cov():
        tomo.covariance(px, py, s.subapd, stars, stars, lay)
    for label, fn, r in (("trace", trace, reps), ("trace + measure", both, reps), ("control", sen.control, reps),
                         ("covariance C_SS %d^2" % (K * ns), cov, 1)):
        med, lo, hi = timed(fn, r, rounds)
        print("%-34s %4d sub-apertures x %3d environments x %d stars  %-24s %9.3f ms  (%.3f .. %.3f over %d rounds of %d)"
              % (name, s.nvalid, nenv, K, label, med, lo, hi, rounds, r))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args(argv)
    if not a.no_large:
        run("production_sh_40x40_8m_3layers", 256, a.reps, a.rounds)
    run("production_sh_10x10_2m", 64, a.reps, a.rounds)


if __name__ == "__main__":
    main()
