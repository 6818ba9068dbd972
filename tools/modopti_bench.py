"""Times the modal-gain filter bank (aomarl_modopti_*, ao_marl_amd.modal_gains.NativeLoopBank) at the production size --
256 environments x 1283 modes x 15 gains over 2048 frames, fed in chunks of 64 -- against the same recursion written
with float64 torch tensors on the device (one elementwise pass per frame over [nenv][nmodes][ngain]).

    python tools/modopti_bench.py [--nenv 256] [--nmodes 1283] [--ngain 15] [--frames 2048] [--chunk 64] [--reps 3]
                                  [--torch-frames 256]

No loop is run: the series is a random walk, what the kernel costs does not depend on the values.  The torch statement
is timed over --torch-frames frames and scaled to --frames.  Prints the time per call of aomarl_modopti_accumulate, the
whole series, frames x series x gains per second, and the bytes of x and of filter state moved per second.

    python tools/modopti_bench.py --online [--steps 200] [--warmup 20] [--period 256]

times one frame of the general chain under modal gains (aomarl_env_step with zero actions), the on-line optimiser
(modal_gains.OnlineModalGains) off against attached, at 10x10 / 64 environments and 40x40 / 256 environments: what the
extra product v2m . voltage, k_mo_pol and the amortised bank and apply cost per frame."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def online(a):
    """time per frame of the general chain, optimiser off / attached"""
    import torch
    from ao_marl_amd import modal_gains as mg
    from ao_marl_amd import params
    from ao_marl_amd.env import VecAoEnv
    small = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
    large = dict(n_zernike_start_end=[0, 1274], n_reverse_filtered_from_cmat=5, window_n_zernike=20,
                 include_tip_tilt_windowed=True)
    for name, nenv, rl, nag in (("production_sh_10x10_2m", 64, small, 1), ("production_sh_40x40_8m_3layers", 256, large, 13)):
        env = VecAoEnv(params.builtin(name), nenv, rl, n_agents_modal=nag, frame_pipeline=False)
        sup = env.supervisor
        sup.set_modal_gains(np.ones(sup.nmodes, dtype=np.float32))
        zero = torch.zeros(nenv, env.action_dim, device="cuda:0")

        def per_frame():
            env.reset()
            for _ in range(a.warmup):
                env.step(zero)
            torch.cuda.synchronize()
            best = 1e30
            for _ in range(a.reps):
                t = time.perf_counter()
                for _ in range(a.steps):
                    env.step(zero)
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t) / a.steps)
            return best
        off = per_frame()
        opt = mg.OnlineModalGains(sup, nskip=50, period=a.period, horizon=2048, pool="all").start()
        on = per_frame()
        nup = opt.updates
        opt.stop()
        print("online  %s, %d environments, %d modes, 15 gains, period %d: %.3f ms per frame off, %.3f ms attached "
              "(+%.3f ms, %+.1f %%; %d applies)" % (name, nenv, sup.nmodes, a.period, 1e3 * off, 1e3 * on, 1e3 * (on - off),
                                                   100.0 * (on - off) / off, nup), flush=True)
        del env, sup, opt


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
    ap.add_argument("--online", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--period", type=int, default=256)
    a = ap.parse_args(argv)
    if a.online:
        return online(a)
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
