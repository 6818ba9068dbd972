#!/usr/bin/env python3
"""Timing of the denoiser's training step and of paired recording (not part of bench.py).

  python tools/denoiser_train_bench.py [--batches 256,4096,65536] [--repeats 7] [--record]

Per batch size: the native step (aomarl_denoiser_trainer_step) against the tensor-library autograd
step (DenoiserTrainer(native=False) on the same GPU, MIOpen convolutions), device events around
`inner` back-to-back steps, median and spread over `repeats` after a warm-up; images / s, GFLOP/s by
the 10.3 MFLOP-per-image count (1 712 128 MAC forward, twice more backward) and the fraction of the
fp32 matrix peak.  --record: record_pairs per frame against the plain noisy step of the loop.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ao_marl_amd import denoiser as D  # noqa: E402

FLOP_PER_IMAGE = 3 * 2 * 1712128          # forward, input gradients, weight gradients
PEAK_F32_MATRIX = 157.3e12                # MI355X: fp32 matrix instructions, FLOP/s


def timed(fn, inner, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096,65536")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--config", default="production_sh_40x40_8m_3layers_d0_noise")
    ap.add_argument("--nenv", type=int, default=16)
    args = ap.parse_args()
    dev = "cuda:0"
    for batch in [int(b) for b in args.batches.split(",") if b]:
        n, c = (t.to(dev) for t in D.synthetic_pairs(batch, seed=1))
        # a timed window of a quarter of a million images: long against the launch overhead and the clock at every size
        inner = max(2, min(400, 262144 // batch))
        row = {"what": "train_step", "batch": batch, "inner": inner, "repeats": args.repeats}
        for name, native in (("native", True), ("autograd", False)):
            tr = D.DenoiserTrainer(None, device=dev, seed=1, native=native, max_batch=batch)
            med, lo, hi = timed(lambda: tr.step(n, c), inner, args.repeats)
            row[name + "_ms"] = round(med, 4)
            row[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            row[name + "_images_per_s"] = round(batch / med * 1e3)
            flops = batch * FLOP_PER_IMAGE / (med * 1e-3)
            row[name + "_gflops"] = round(flops / 1e9, 1)
            row[name + "_fraction_of_f32_matrix_peak"] = round(flops / PEAK_F32_MATRIX, 4)
            del tr
        row["speedup"] = round(row["autograd_ms"] / row["native_ms"], 3)
        print(json.dumps(row), flush=True)
    if args.record:
        from ao_marl_amd.env import VecRlSupervisor
        sup = VecRlSupervisor(args.config, {}, args.nenv, prefetch_atmos=False)
        sup.reset()

        def plain():
            sup.next_part_one()
            sup.next_part_two(None, linear_control=True)

        p = timed(plain, 10, args.repeats)
        r = timed(lambda: D.record_pairs(sup, 10, reset=False), 1, args.repeats)
        print(json.dumps({"what": "record_pairs", "config": args.config, "nenv": args.nenv,
                          "plain_ms_per_frame": round(p[0], 4), "plain_ms_min_max": [round(p[1], 4), round(p[2], 4)],
                          "record_ms_per_frame": round(r[0] / 10, 4),
                          "record_ms_min_max": [round(r[1] / 10, 4), round(r[2] / 10, 4)]}), flush=True)


if __name__ == "__main__":
    main()
