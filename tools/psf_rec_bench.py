"""Timing of the PSF reconstruction (ao_marl_amd.psf_rec.ViiReconstructor) at the sizes of the two production systems,
on synthetic systems of the same shape (Gaussian influence functions, about 8 taps per pixel) with random covariances:

    python tools/psf_rec_bench.py [--sizes 10x10 40x40] [--repeat 3] [--numpy-modes 8]

Per size: the device's accumulate + finish (HIP events around the library calls, the host's eigendecomposition timed
apart), transforms per second, the memory traffic predicted per mode and the bandwidth that makes of it; the same loop
written with torch.fft on the same GPU (the vendor's FFT: a yardstick, never on the product's path); the float64 NumPy
restatement on the host, timed on --numpy-modes modes and scaled to all of them."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"10x10": dict(p=160, side=9, nmodes=87, extra=7), "40x40": dict(p=640, side=36, nmodes=1283, extra=-12)}
HBM_PEAK = 8.0e12          # bytes / s, MI355X


def system(p, side, nmodes, extra, seed=0):
    """side^2 + extra + 2 actuators (extra < 0 drops some), nmodes modes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:p, :p] - (p - 1) / 2.0
    spup = (np.hypot(x, y) <= p / 2.0).astype(np.float64)
    idx = -np.ones(p * p, dtype=np.int64)
    lit = np.flatnonzero(spup.ravel())
    idx[lit] = np.arange(lit.size)
    g = np.linspace(-1.0, 1.0, side) * p / 2 + (p - 1) / 2.0
    pitch = g[1] - g[0]
    half = int(np.ceil(1.55 * pitch))
    rows, cols, vals = [], [], []
    acts = [(cy, cx) for cy in g for cx in g][:side * side + min(extra, 0)]
    acts += [(g[side // 2] + 0.5 * pitch, g[k % side] + 0.5 * pitch) for k in range(max(extra, 0))]
    for a, (cy, cx) in enumerate(acts):
        ys = np.arange(max(int(cy) - half, 0), min(int(cy) + half + 1, p))
        xs = np.arange(max(int(cx) - half, 0), min(int(cx) + half + 1, p))
        Y, X = np.meshgrid(ys, xs, indexing="ij")
        r2 = (Y - cy) ** 2 + (X - cx) ** 2
        k = idx[(Y * p + X).ravel()]
        ok = (k >= 0) & (r2.ravel() <= (1.55 * pitch) ** 2)
        rows.append(np.full(int(ok.sum()), a))
        cols.append(k[ok])
        vals.append(np.exp(-r2.ravel()[ok] / (0.7 * pitch) ** 2))
    nact = len(acts)
    IF = sp.csr_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(cols))),
                       shape=(nact, lit.size))
    TT = (np.stack([x.ravel()[lit], y.ravel()[lit]], axis=1) / (p / 2.0)).astype(np.float32)
    Btt = rng.normal(size=(nact + 2, nmodes)) / np.sqrt(nact)
    y_ = rng.normal(size=(nmodes, 2 * nmodes)) * 0.02
    return spup, IF, TT, Btt, y_.dot(y_.T) / y_.shape[1]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["10x10", "40x40"], choices=sorted(SIZES))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--numpy-modes", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    import torch
    from ao_marl_amd import psf_rec
    for name in a.sizes:
        spup, IF, TT, Btt, cov = system(**SIZES[name])
        taps = np.asarray((IF != 0).sum(axis=0)).ravel()
        rec = psf_rec.ViiReconstructor(spup, IF, TT, Btt, 1.65, device=a.device)
        p, N, nk = rec.p, rec.N, cov.shape[0]
        t0 = time.perf_counter()
        com, w = rec.modes_of(cov)
        t_eig = time.perf_counter() - t0
        dev = torch.device(a.device)
        com_d = torch.as_tensor(com.astype(np.float32), device=dev)
        w_d = torch.as_tensor(w.astype(np.float32), device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        best_acc = best_fin = float("inf")
        for _ in range(a.repeat + 1):                                    # the first pass warms up
            rec.reset()
            ev[0].record()
            rec.accumulate(com_d, w_d)
            ev[1].record()
            out = rec.finish()
            ev[2].record()
            torch.cuda.synchronize()
            best_acc, best_fin = min(best_acc, ev[0].elapsed_time(ev[1]) * 1e-3), min(best_fin, ev[1].elapsed_time(ev[2]) * 1e-3)
        nc, rows = N // 2 + 1, 2 * ((p + 1) // 2)
        per_mode = 2 * p * p * 4 + rows * nc * 8 + p * nc * 8            # map written and read, T written and read
        print("%s: p = %d, N = %d, %d modes, %d lit pixels, taps per pixel max %d mean %.1f" %
              (name, p, N, nk, rec.npts, taps.max(), taps.mean()))
        print("  device   accumulate %.4f s (%.0f transforms / s), finish %.4f s, eigh + Btt V on the host %.3f s, Strehl %.4f"
              % (best_acc, nk / best_acc, best_fin, t_eig, float(out[2].max())))
        print("  traffic  %.2f MB predicted per mode -> %.0f GB/s, %.1f %% of %.0f TB/s" %
              (per_mode / 1e6, per_mode * nk / best_acc / 1e9, 100 * per_mode * nk / best_acc / HBM_PEAK, HBM_PEAK / 1e12))
        # the same loop on the vendor's FFT through torch
        maps = torch.as_tensor(rec.maps_of(com[:16]).astype(np.float32), device=dev)
        yy, xx = (torch.as_tensor(v, device=dev) for v in np.divmod(rec.lit.astype(np.int64), p))
        grid = torch.zeros(16, p, p, device=dev)
        grid[:, yy, xx] = maps
        acc = torch.zeros(N, nc, device=dev)
        best = float("inf")
        for _ in range(a.repeat + 1):
            ev[0].record()
            for k0 in range(0, nk, 16):
                nb = min(16, nk - k0)
                F = torch.fft.rfft2(grid[:nb], s=(N, N))
                acc += (w_d[k0:k0 + nb, None, None] * (F.real ** 2 + F.imag ** 2)).sum(0)
            ev[1].record()
            torch.cuda.synchronize()
            best = min(best, ev[0].elapsed_time(ev[1]) * 1e-3)
        print("  torch.fft on the same GPU (transforms and sum only, maps given) %.4f s (%.0f transforms / s)" % (best, nk / best))
        # float64 NumPy on the host, a few modes
        nm = min(a.numpy_modes, nk)
        t0 = time.perf_counter()
        np.linalg.eigvalsh(cov)                                           # what the full run would add
        t_e = time.perf_counter() - t0
        grid64, fp = np.zeros((N, N)), np.fft.fft2(rec.tel["pup"])
        m = rec.maps_of(com[:nm])
        t0 = time.perf_counter()
        for k in range(nm):
            grid64[np.divmod(rec.lit, p)] = m[k]
            _ = (np.fft.fft2(grid64 * grid64) * np.conj(fp)).real - np.abs(np.fft.fft2(grid64)) ** 2
        t_np = (time.perf_counter() - t0) / nm
        print("  float64 NumPy restatement on the host: %.4f s per mode (%d timed) -> %.1f s for %d modes (+ eig %.2f s)" %
              (t_np, nm, t_np * nk, nk, t_e))
        del rec


if __name__ == "__main__":
    main()
