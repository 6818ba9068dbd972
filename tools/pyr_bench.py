"""Times a measure of the pyramid sensor (ao_marl_amd.pyramid.NativePyramid, csrc/aomarl_pyr.hip) on the device:

    python tools/pyr_bench.py [--reps 20] [--large-envs 4] [--no-large]

  10x10 / 2 m at nxsub 20 (Nfft 512, n 164), 64 environments, 16 modulation points
  40x40 / 8 m at nxsub 40 (Nfft 2048, n 644), --large-envs environments, 16 modulation points

Per shape: ms per measure (device events around `reps` measures, the first one not counted), GFLOP/s by the
5 N log2 N count of the transforms a measure asks for (per pair: n + 2 Nfft + Nfft lines; with the pixel filter
4 Nfft lines per environment), and the bytes the three passes move through memory (their reads and writes of the
intermediate planes, the image and the filter's planes; nothing that stays in LDS).  The phases are random; the time
does not depend on them.  No threshold: the figures go into LAB_NOTEBOOK.md."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def geometry(pupdiam, diam, nxsub):
    from ao_marl_amd import geometry as G, params as P
    tel = P.Param_tel(diam=diam, cobs=0.12)
    w = P.Param_wfs(type="pyrhr", nxsub=nxsub, pyr_ampl=3., pyr_npts=16, fstop="round", Lambda=0.5, gsmag=4., noise=-1.,
                    fssize=nxsub * 0.5e-6 / diam * G.RAD2ARCSEC, optthroughput=0.12, zerop=1e11, fracsub=0.8)
    geom = G.pupil_geometry(pupdiam, tel)
    return G.pyr_geometry(w, G.pyr_sizes(w, tel, geom.pupdiam), geom, tel, 0.002)


def counts(pg, nenv, npts, pixel_filter):
    """(flop, bytes) of one measure"""
    N, n = pg.Nfft, pg.n
    line = 5.0 * N * math.log2(N)
    pairs = nenv * npts
    flop = pairs * (n + 2 * N + N) * line + (4 * N * line * nenv if pixel_filter else 0)
    t1, t2 = 8.0 * n * N, 8.0 * N * N
    byt = pairs * (4.0 * n * n + t1            # rows: the phase in, T1 out
                   + t1 + t2 + t2              # columns: T1 and the mask in, T2 out
                   + t2)                       # inverse rows: T2 in
    byt += nenv * 4.0 * N * N * 2              # the image out, and in again for the binning
    if pixel_filter:
        byt += nenv * (4.0 * N * N * 2 + 6 * t2 + 4.0 * N * N)
    return flop, byt


def run(name, pg, nenv, reps, pixel_filter=True):
    import torch
    from ao_marl_amd.pyramid import NativePyramid
    nat = NativePyramid(pg, nenv, pixel_filter=pixel_filter)
    npts = int(np.size(pg.pyr_cx))
    nat.set_modulation(pg.pyr_cx, pg.pyr_cy, np.ones(npts), pg.s_scale)
    ph = 0.1 * torch.randn(nenv, pg.n, pg.n, device=nat.device)
    nat.measure(ph)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        nat.measure(ph)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / reps
    flop, byt = counts(pg, nenv, npts, pixel_filter)
    print("%-34s Nfft %4d  n %3d  %3d environments x %2d points  filter %d: %9.3f ms / measure  %8.1f GFLOP/s  "
          "%7.1f MB moved  %7.1f GB/s" % (name, pg.Nfft, pg.n, nenv, npts, int(pixel_filter), ms, flop / ms / 1e6,
                                          byt / 1e6, byt / ms / 1e6))
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--large-envs", type=int, default=4)
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args(argv)
    small = geometry(160, 2.0, 20)
    run("10x10 / 2 m, nxsub 20", small, 64, a.reps)
    run("10x10 / 2 m, nxsub 20, no filter", small, 64, a.reps, pixel_filter=False)
    if not a.no_large:
        run("40x40 / 8 m, nxsub 40", geometry(640, 8.0, 40), a.large_envs, max(1, a.reps // 4))


if __name__ == "__main__":
    main()
