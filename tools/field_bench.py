"""Times the science field (ao_marl_amd.field, csrc/aomarl_field.hip) on the device:

    python tools/field_bench.py [--reps 20] [--rounds 5] [--halfwin 8] [--no-large]

  40x40 / 8 m, three layers, 256 environments        10x10 / 2 m, 64 environments        field declared at 25 arcsec

Per shape and per T = 1, 9 (a 3 x 3 grid over +-20 arcsec) and 16 (a ring at 20 arcsec), ms per call:
  observe            aomarl_field_observe: trace, window, variance, fit and commit of the T directions of every environment
  T x on-axis        the yardstick: T back-to-back calls of today's on-axis aomarl_target_psf + aomarl_comp_strehl on the
                     same state (whole-pixel offsets: one tap per layer where the field gathers four)
  trace              aomarl_field_trace: the T planes alone
Device events around `reps` calls, `rounds` times: the median and the spread (min .. max) of the rounds.  No threshold:
the figures go into DESIGN.md."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.lgs_bench import timed  # noqa: E402


def run(name, nenv, reps, rounds, halfwin, field=25.):
    import torch
    from ao_marl_amd import field as F, geometry as G, params as P, system
    from ao_marl_amd.sim import HipSim
    from ao_marl_amd.tomography import with_field
    ps = with_field(P.builtin(name), field)
    sysm = G.build_system(ps)
    s = system.from_system(sysm, strehl_halfwin=halfwin)
    sim = HipSim(s, nenv=nenv)
    sim.reset(np.arange(nenv) + 1234)
    rng = np.random.default_rng(1)
    sim.comp_dm_shape(torch.as_tensor(0.05 * rng.normal(size=(nenv, s.nactu)).astype(np.float32), device=sim.device))
    for T, dirs in ((1, [(0., 0.)]), (9, F.grid(20., 3)), (16, F.ring(16, 20.))):
        fld = F.ScienceField(sim, dirs, sysm=sysm)
        planes = torch.zeros(nenv, T, s.pupdiam, s.pupdiam, dtype=torch.float32, device=sim.device)

        def yardstick():
            for _ in range(T):
                sim.target_psf()
                sim.comp_strehl()
        for label, fn in (("observe", fld.native.observe), ("%d x on-axis psf + strehl" % T, yardstick),
                          ("trace", lambda: fld.native.trace(planes))):
            med, lo, hi = timed(fn, reps, rounds)
            print("%-34s pupil %3d, window %2d x %3d environments x %2d directions  %-26s %9.3f ms  (%.3f .. %.3f over %d rounds of %d)"
                  % (name, s.pupdiam, 2 * halfwin, nenv, T, label, med, lo, hi, rounds, reps))
        del fld, planes


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--halfwin", type=int, default=8, help="strehl_halfwin (VecAoEnv's is 8)")
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args(argv)
    if not a.no_large:
        run("production_sh_40x40_8m_3layers", 256, a.reps, a.rounds, a.halfwin)
    run("production_sh_10x10_2m", 64, a.reps, a.rounds, a.halfwin)


if __name__ == "__main__":
    main()
