"""Times the laser-guide-star sensor (ao_marl_amd.lgs.NativeLgs, csrc/aomarl_lgs.hip) on the device, beside the existing
Shack-Hartmann image of the same simulator in the same command:

    python tools/lgs_bench.py [--reps 20] [--rounds 5] [--no-large]

  40x40 / 8 m, three layers, 256 environments        10x10 / 2 m, 64 environments

Per shape: ms per `trace + measure` of the LGS (the cone trace into the phase buffer, then image, binning, flux, centre of
gravity; noise off, side launch) and ms per `comp_image` of the NGS Shack-Hartmann (its own trace, image and centre of
gravity; noise off).  Device events around `reps` calls, `rounds` times: the median and the spread (min .. max) of the
rounds.  The screens are a fresh reset; the time does not depend on them.  No threshold: the figures go into DESIGN.md."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, rounds):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def run(name, nenv, reps, rounds, gsalt=90e3):
    from ao_marl_amd import geometry as G, lgs as L, params as P, system
    from ao_marl_amd.sim import HipSim
    ps = P.builtin(name)
    sysm = G.build_system(ps)
    s = system.from_system(sysm)
    sim = HipSim(s, nenv=nenv, keep_phase=True)
    sim.reset(np.arange(nenv) + 1234)
    w = sysm.wfss[0]
    alt, prof = L.lgs_profile("gauss1")
    K = L.lgs_kernels(w, w, ps.p_tel, alt, prof, -ps.p_tel.diam, 0., 0.8)
    nat = L.NativeLgs(s, nenv, K, noise=-1.)
    deltas = L.cone_deltas(sysm.atm.alt, gsalt)

    def lgs():
        nat.trace(sim, deltas)
        nat.measure(sim.t["wfs_phase"], write_cube=False)

    def trace():
        nat.trace(sim, deltas)

    def sh():
        sim.comp_image(noise=False, write_bincube=False, cog=True)
    for label, fn in (("LGS trace + measure", lgs), ("LGS trace alone", trace), ("SH comp_image", sh)):
        med, lo, hi = timed(fn, reps, rounds)
        print("%-34s %4d sub-apertures x %3d environments  %-20s %8.3f ms  (%.3f .. %.3f over %d rounds of %d)"
              % (name, s.nvalid, nenv, label, med, lo, hi, rounds, reps))


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
