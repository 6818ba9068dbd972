"""Times the modal predictor's kernel (k_pred_step, aomarl_predictor_push, ao_marl_amd.predictive.NativePredictorBank)
alone at the production size -- 256 environments x 1283 modes -- for orders 1, 2, 4, 8: ms per frame of one-frame
calls (what aomarl_do_control pays per frame while one is attached), learning and frozen, by device events, and the
same per frame inside one call of --chunk frames (the state loaded once: what a warm start pays).

    python tools/predictor_bench.py [--nenv 256] [--nmodes 1283] [--orders 1 2 4 8] [--frames 200] [--warmup 20]
                                    [--reps 3] [--chunk 64] [--horizon 2048]

No loop is run: the series is coloured noise, what the kernel costs does not depend on the values.  Beside each time:
the bytes the state moves per frame -- theta, the upper triangle of P, the order + 2 past values, J and J0 in double, read
and written once, plus the x row read and the two c rows written in float32 -- and the rate that makes.

    python tools/predictor_bench.py --step [--steps 200]

times one frame of the general chain at 40x40 / 256 environments (aomarl_env_step with zero actions) under modal gains
against the same with a predictor of each order attached."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def state_bytes(order, nseries, learning=True):
    """bytes one frame moves: the state read and written once (P only while learning), x in, c out twice"""
    slots = order + (order * (order + 1) // 2 if learning else 0) + order + 2 + 2
    return nseries * (2 * 8 * slots + 3 * 4)


def step(a):
    """time per frame of the general chain, the integrator under modal gains / the predictor attached"""
    import torch
    from ao_marl_amd import params, predictive as pc
    from ao_marl_amd.env import VecAoEnv
    large = dict(n_zernike_start_end=[0, 1274], n_reverse_filtered_from_cmat=5, window_n_zernike=20,
                 include_tip_tilt_windowed=True)
    name, nenv = "production_sh_40x40_8m_3layers", a.nenv
    env = VecAoEnv(params.builtin(name), nenv, large, n_agents_modal=13, frame_pipeline=False)
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
    print("step    %s, %d environments, %d modes: %.3f ms per frame under modal gains (the integrator)" %
          (name, nenv, sup.nmodes, 1e3 * off), flush=True)
    for order in a.orders:
        pred = pc.ModalPredictor(sup, order=order, horizon=a.horizon).start()
        on = per_frame()
        pred.stop()
        print("step    predictor of order %d attached: %.3f ms per frame (%+.3f ms, %+.1f %%)" %
              (order, 1e3 * on, 1e3 * (on - off), 100.0 * (on - off) / off), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nenv", type=int, default=256)
    ap.add_argument("--nmodes", type=int, default=1283)
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--horizon", type=float, default=2048.0)
    ap.add_argument("--delay", type=float, default=1.0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args(argv)
    if a.step:
        return step(a)
    import torch
    from ao_marl_amd import libaomarl as la
    from ao_marl_amd import predictive as pc
    dev = torch.device("cuda:0")
    stream = la.raw_stream(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(a.chunk, a.nenv, a.nmodes, device=dev, generator=g)
    x = (x + torch.roll(x, 1, 0) + torch.roll(x, 2, 0)).contiguous()
    ns = a.nenv * a.nmodes
    forget = float(np.exp(-1.0 / a.horizon)) if a.horizon else 1.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, n):
        """best of --reps: ms per frame of n frames issued by fn, by device events"""
        best = 1e30
        for _ in range(a.reps):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / n)
        return best
    for order in a.orders:
        bank = pc.NativePredictorBank(a.nenv, a.nmodes, order, a.delay, forget, 1e4, 50, device=dev)
        c = torch.empty(1, a.nenv, a.nmodes, device=dev)

        def frames():
            for t in range(a.frames):
                bank.lib.aomarl_predictor_push(bank.ptr, x[t % a.chunk].data_ptr(), 1, ns, c.data_ptr(), stream)
        for t in range(a.warmup):
            bank.push(x[t % a.chunk:t % a.chunk + 1])
        torch.cuda.synchronize()
        for learning in (True, False):
            bank.learning = learning
            ms = timed(frames, a.frames)
            by = state_bytes(order, ns, learning)
            print("kernel  order %d, %d x %d series, forget %.6f, %s: %.4f ms per frame; %.1f MB of state and rows per "
                  "frame: %.0f GB / s" % (order, a.nenv, a.nmodes, forget, "learning" if learning else "frozen  ", ms,
                                          by / 1e6, by / ms / 1e6), flush=True)
        bank.learning = True
        ms = timed(lambda: bank.push(x, want_c=False), a.chunk)
        print("kernel  order %d, one call of %d frames (the state loaded once): %.4f ms per frame" % (order, a.chunk, ms),
              flush=True)
        del bank


if __name__ == "__main__":
    main()
