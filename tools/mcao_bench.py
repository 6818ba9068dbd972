"""Times multi-conjugate AO (ao_marl_amd.mcao, csrc/aomarl_mcao.hip) on the device:

    python tools/mcao_bench.py [--reps 20] [--rounds 5] [--no-large]

  40x40 / 8 m, three layers, 256 environments, mirrors at 4500 and 14000 m
  10x10 / 2 m, 64 environments, one mirror at 8000 m                        K = 4 stars at 90 km, 20 arcsec, field 25 arcsec

Per shape, ms per call:
  apply              aomarl_mcao_apply: the delay line (k_mcao_apply) and every mirror's plane (k_mcao_shape)
  add, K = 4         aomarl_mcao_add on the stars' planes (k_mcao_add<4>)
  add, target        aomarl_mcao_add on the state's tar_phase (k_mcao_add<1>, the pupil grid)
  frame, attached    MultiConjugate.frame() + control() + apply(): what next_part_one / next_part_two run per step
  frame, parent      LaserTomography.frame() + control(): the same without the mirrors at altitude
(matrices of the sensors' shapes filled with small random numbers: the time does not depend on them; noise off.)
Device events around `reps` calls, `rounds` times: the median and the spread (min .. max) of the rounds.  No threshold:
the figures go into DESIGN.md."""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.lgs_bench import timed  # noqa: E402


def run(name, nenv, alts, reps, rounds, K=4, radius=20., field=25.):
    import torch
    from ao_marl_amd import geometry as G, lgs as L, mcao as M, params as P, system, tomography as T
    from ao_marl_amd.sim import HipSim
    ps = T.with_field(P.builtin(name), field)
    sysm = G.build_system(ps)
    s = system.from_system(sysm)
    sim = HipSim(s, nenv=nenv, keep_phase=True)
    sim.reset(np.arange(nenv) + 1234)
    stars = T.ring(K, radius)
    con = T.Constellation(stars)
    off, dm1, _ = T.constellation_offsets(sysm, stars)
    w = sysm.wfss[0]
    alt, prof = L.lgs_profile("gauss1")
    kern = L.lgs_kernels(w, w, ps.p_tel, alt, prof, 0., 0., 0.8)
    mirrors = [M.altitude_mirror(sysm, h, field) for h in alts]
    ns, na = 2 * s.nvalid, s.nactu
    g = torch.Generator(device="cuda:0").manual_seed(1)
    rnd = lambda *sh: 1e-3 * torch.randn(*sh, device="cuda:0", generator=g)  # noqa: E731
    sup = types.SimpleNamespace(sim=sim, gain=0.5, prefetch_atmos=False, keep_wfs_phase=False)

    def sensor(cls):
        # the sensor's frame() and control() on buffers of its shapes (no calibration: the matrices of a 40x40 system are
        # minutes of host algebra)
        sen = cls.__new__(cls)
        sen.sup, sen.s, sen.tomo, sen.polc = sup, s, T.NativeTomo(), True
        sen.native = L.NativeLgs(s, nenv * K, kern, noise=-1.)
        sen.nenv, sen.K, sen.nslope, sen.off, sen.dm1 = nenv, K, ns, off, dm1
        sen.planes = torch.zeros(nenv, K, s.n, s.n, dtype=torch.float32, device="cuda:0")
        sen.est = torch.zeros(nenv, ns, device="cuda:0")
        sen._dev = [rnd(na, K * ns), rnd(ns, K * ns), rnd(na, int(sim._frame_buf("voltage").shape[1]))]
        return sen
    parent = sensor(T.LaserTomography)
    mc = sensor(M.MultiConjugate)
    mc.mirrors, mc.M, mc.reconstructor = mirrors, len(mirrors), "ls"
    mc.mc = nm = M.NativeMcao(sim, mirrors)
    mc.nact_total = nm.nact_total
    mc.wfs_view = M.mirror_offsets(sysm, mirrors, con, "wfs")
    mc.sci_view = M.mirror_offsets(sysm, mirrors, [(0., 0.)], "pupil")
    mc._ls_dev = [rnd(na, K * ns), rnd(nm.nact_total, K * ns)]
    mc._alt_err = torch.zeros(nenv, nm.nact_total, device="cuda:0")
    nm.com.copy_(30. * torch.randn(nenv, nm.nact_total, device="cuda:0", generator=g))
    sim._need_phase()

    def attached():
        mc.frame(False)
        mc.control()
        mc.apply()

    def plain():
        parent.frame(False)
        parent.control()
    shape = "%s  %d environments, mirrors at %s m (%s actuators, planes of %s pixels)" % (
        name, nenv, "/".join("%g" % h for h in alts), "+".join(str(m.ntotact) for m in mirrors), "/".join(str(m.dim) for m in mirrors))
    for label, fn in (("apply", nm.apply), ("add, K = %d" % K, lambda: nm.add(*mc.wfs_view, mc.planes)),
                      ("add, target", lambda: nm.add(*mc.sci_view, sim.t["tar_phase"])), ("frame, attached", attached),
                      ("frame, parent", plain)):
        med, lo, hi = timed(fn, reps, rounds)
        print("%s  %-18s %9.3f ms  (%.3f .. %.3f over %d rounds of %d)" % (shape, label, med, lo, hi, rounds, reps), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args(argv)
    run("production_sh_10x10_2m", 64, (8000.,), a.reps, a.rounds)
    if not a.no_large:
        run("production_sh_40x40_8m_3layers", 256, (4500., 14000.), a.reps, a.rounds)


if __name__ == "__main__":
    main()
