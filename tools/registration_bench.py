"""Times the registered ray trace (ao_marl_amd.registration, csrc/aomarl_capi_dmreg.hip: k_trace_reg) on the device
against the plain one (aomarl_raytrace_wfs / _target: k_raytrace) on the same state:

    python tools/registration_bench.py [--config production_sh_40x40_8m_3layers] [--envs 256] [--reps 50] [--rounds 9]
                                       [--loop-frames 0]

Per grid (sensor, target) three variants alternate within every round -- the plain trace, the registered trace with the
identity table, the registered trace with 1 degree / 0.3 pitch on the stack-array mirror --, each timed with device
events around `reps` calls; the figure is the median over the rounds, the spread their range.  The bar: the identity
trace is no slower than the plain one beyond the spread of the plain one measured in this same command.

Bytes per call come from shapes (registration.trace_bytes: the windows of the screens, the windows of the mirrors' planes,
one store of the grid), the rate is those bytes over the call time, the share is of the 8.0 TB/s HBM peak; the traffic is
the memory system's to bound, not the arithmetic (about 60 flops a pixel against 20 bytes).  Call time includes the
launch; kernel time is a separate run under rocprofv3 --kernel-trace --stats (kernels: k_trace_reg, k_raytrace).

--loop-frames N also builds the supervisor of the configuration (calibration included) and reports closed-loop frames
per second over N frames with a registration attached beside the stage-by-stage call order without one."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def counts(s, nenv, target):
    """(bytes per call, of which shared by all environments) from shapes"""
    from ao_marl_amd import registration as R
    per_env, shared = R.trace_bytes(s, target)
    return per_env * nenv + shared, shared


def time_variants(variants, reps, rounds):
    """{name: [ms per call, one per round]}; the variants alternate inside every round"""
    import torch
    out = {name: [] for name, _ in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, fn in variants:                   # every shape warm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants:
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps)
    return out


def traces(a):
    import torch
    from ao_marl_amd import geometry as G, params as P, registration as R, system
    from ao_marl_amd.sim import HipSim
    sysm = G.build_system(P.builtin(a.config))
    s = system.from_system(sysm)
    sim = HipSim(s, nenv=a.envs, keep_phase=True)
    sim.reset(1234 + 16 * np.arange(a.envs))
    sim.move_atmos()
    sim.comp_dm_shape(0.3 * torch.randn(a.envs, s.nactu, device=sim.device))
    reg = R.NativeRegistration(sim)
    ident = np.tile(R.IDENTITY_ROW, (a.envs, 1))
    A, t = R.registration_affine(0.3 * float(s.dms[0].pitch), 0.0, np.deg2rad(1.0), 1.0, 1.0)       # in pixels
    moved = np.tile(R.rows_of(A, t), (a.envs, 1))
    print("%s, %d environments, n %d, pupdiam %d, %d layers, mirrors %s; %d calls per timing, %d rounds" %
          (a.config, a.envs, s.n, s.pupdiam, s.nscreens, [(d.type, d.dim) for d in s.dms], a.reps, a.rounds))
    ok = True
    for target in (False, True):
        plain = sim.raytrace_target if target else sim.raytrace_wfs

        def registered():
            reg.trace(target)
        results = {}
        for name, rows in (("identity", ident), ("1 deg / 0.3 pitch", moved)):
            reg.set_rows(0, rows)
            res = time_variants([("plain", plain), (name, registered)], a.reps, a.rounds)
            results.setdefault("plain", []).extend(res["plain"])
            results[name] = res[name]
        byt, shared = counts(s, a.envs, target)
        med = {k: float(np.median(v)) for k, v in results.items()}
        spread = {k: float(np.max(v) - np.min(v)) for k, v in results.items()}
        for k in ("plain", "identity", "1 deg / 0.3 pitch"):
            print("%-7s %-18s %8.4f ms / call  (range %.4f over %d timings)  %7.1f MB by shapes  %7.1f GB/s  %5.1f %% of the "
                  "HBM peak" % ("target" if target else "sensor", k, med[k], spread[k], len(results[k]), byt / 1e6,
                                byt / med[k] / 1e6, 100.0 * byt / (med[k] * 1e-3) / HBM_PEAK))
        held = med["identity"] <= med["plain"] + spread["plain"]
        print("%-7s bar (identity no slower than plain beyond plain's spread): %s" % ("target" if target else "sensor",
                                                                                      "held" if held else "MISSED"))
        ok = ok and held
    return ok


def loop(a):
    import torch
    from ao_marl_amd import registration as R
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(a.config, dict(n_reverse_filtered_from_cmat=5), a.envs)

    def rate():
        sup.reset()
        sup.next_part_one()
        for _ in range(10):
            sup.next_part_two(None, linear_control=True)
            sup.next_part_one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.loop_frames):
            sup.next_part_two(None, linear_control=True)
            sup.next_part_one()
        torch.cuda.synchronize()
        return a.loop_frames / (time.perf_counter() - t0)
    sup.next_part_one_split = True
    plain = rate()
    reg = R.DmRegistration(sup)
    reg.randomize(1, shift_sigma_m=0.1 * float(sup.s.dms[0].pitch) * reg.pixsize, theta_sigma=np.deg2rad(0.5), G_sigma=0.01)
    reg.start()
    attached = rate()
    reg.stop()
    print("closed loop, %d frames of %d environments: %.1f frames/s stage by stage without a registration, %.1f frames/s "
          "with one attached" % (a.loop_frames, a.envs, plain, attached))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="production_sh_40x40_8m_3layers")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--loop-frames", type=int, default=0)
    a = ap.parse_args(argv)
    ok = traces(a)
    if a.loop_frames > 0:
        loop(a)
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
