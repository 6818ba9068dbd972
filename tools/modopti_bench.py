"""Times the modal-gain filter bank (aomarl_modopti_*, ao_marl_amd.modal_gains.NativeLoopBank) at the production size --
256 environments x 1283 modes x 15 gains over 2048 frames, fed in chunks of 64 -- against the same recursion written
with float64 torch tensors on the device (one elementwise pass per frame over [nenv][nmodes][ngain]).

    python tools/modopti_bench.py [--nenv 256] [--nmodes 1283] [--ngain 15] [--frames 2048] [--chunk 64] [--reps 3]
                                  [--torch-frames 256]

No loop is run: the series is a random walk, what the kernel costs does not depend on the values.  The torch statement
is timed over --torch-frames frames and scaled to --frames.  Prints the time per call of aomarl_modopti_accumulate, the
whole series, frames x series x gains per second, and the bytes of x and of filter state moved per second."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nenv", type=int, default=256)
    ap.add_argument("--nmodes", type=int, default=1283)
    ap.add_argument("--ngain", type=int, default=15)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-frames", type=int, default=256)
    ap.add_argument("--delay", type=float, default=1.0)
    a = ap.parse_args(argv)
    import torch
    from ao_marl_amd import modal_gains as mg
    dev = torch.device("cuda:0")
    gains = mg.gain_grid(0.0, 1.0, a.ngain)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.cumsum(torch.randn(a.chunk, a.nenv, a.nmodes, device=dev, generator=g), dim=0).contiguous()
    bank = mg.NativeLoopBank(a.nenv, a.nmodes, gains, a.delay, nskip=50, device=dev)
    nchunk = (a.frames + a.chunk - 1) // a.chunk

    def series():
        bank.reset()
        left = a.frames
        for _ in range(nchunk):
            bank.accumulate(x, nframes=min(a.chunk, left))
            left -= a.chunk
    series()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(a.reps):
        t = time.perf_counter()
        series()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    bank.accumulate(x)
    e1.record()
    e1.synchronize()
    call_ms = e0.elapsed_time(e1)
    work = float(a.frames) * a.nenv * a.nmodes * a.ngain
    series_n = a.nenv * a.nmodes
    passes = (a.ngain + 31) // 32
    bytes_moved = nchunk * (2 * 4 * 8 * a.ngain * series_n) + passes * 4.0 * a.frames * series_n
    print("bank    %d x %d x %d gains, %d frames in %d calls: %.2f ms (%.3f ms per call of %d frames by device events)" %
          (a.nenv, a.nmodes, a.ngain, a.frames, nchunk, 1e3 * best, call_ms, a.chunk))
    print("bank    %.2f G filter steps / s, %.1f GB / s of x and filter state" % (work / best / 1e9, bytes_moved / best / 1e9))
    # the statement on the device
    wa, wb, wc = mg.delay_weights(a.delay)
    gt = torch.as_tensor(bank.gains, dtype=torch.float64, device=dev)
    nt = min(a.torch_frames, a.frames)

    def statement():
        c0 = torch.zeros(a.nenv, a.nmodes, a.ngain, dtype=torch.float64, device=dev)
        c1, c2, J = torch.zeros_like(c0), torch.zeros_like(c0), torch.zeros_like(c0)
        for t in range(nt):
            e = x[t % a.chunk].double()[..., None] - (wa * c0 + wb * c1 + wc * c2)
            cn = c0 + gt * e
            if t >= 50:
                J += e * e
            c0, c1, c2 = cn, c0, c1
        return J
    statement()
    torch.cuda.synchronize()
    t = time.perf_counter()
    Jt = statement()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) * a.frames / nt
    print("torch   the same recursion in float64 tensors: %.1f ms for %d frames (timed over %d): bank %.1f x faster" %
          (1e3 * dt, a.frames, nt, dt / best))
    # and the two agree (the bank over the same nt frames)
    bank.reset()
    left = nt
    while left > 0:
        bank.accumulate(x, nframes=min(a.chunk, left))
        left -= a.chunk
    J = bank.result()[0]
    ref = Jt.cpu().numpy()
    ok = mg.pole_radius(bank.gains, a.delay) <= 0.99
    print("check   bank against the torch statement over %d frames: %.2e relative (candidates of pole radius <= 0.99)" %
          (nt, float(np.abs(J[..., ok] - ref[..., ok]).max() / np.abs(ref[..., ok]).max())))


if __name__ == "__main__":
    main()
