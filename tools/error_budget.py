"""ROKET error breakdown of a closed loop (ao_marl_amd.roket.VecRoket) from the command line.

    python tools/error_budget.py --params production_sh_10x10_2m --nenv 4 --frames 300 --preloop 50
    python tools/error_budget.py --params ... --agents 2 --checkpoints DIR     # DIR: one actor file per agent

Without --checkpoints the integrator alone is analysed (6 x 6 tables); with it the agents of the directory (files in
sorted order = agent order, any of the three actor layouts BatchedSAC.load_model accepts) and zeta joins the table.
Prints the reference's progress line every 100 frames and, at the end, the mean over environments of the per-
contributor variance (the diagonal of cov, microns^2), the correlation table, the fitting term, the long-exposure
Strehl and how far exp(-(variance of the sum + fitting)) closes on it.

With --psf-rec the PSF of environment 0 is reconstructed from the covariance of its error buffers (ao_marl_amd.psf_rec,
the reference's gamora.psf_rec_Vii) and its Strehl printed beside the loop's; --psf-rec-out FILE keeps otf2 and psf.

With --groot the bandwidth (+ tomography) variance and the PSF Strehl that the GROOT model (ao_marl_amd.groot) predicts from
wind, r0, L0, gain and guide-star offset alone are printed beside ROKET's measured ones for environment 0: the reference's
groot.test_Cerr.  A comparison, not a check."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--params", default="production_sh_10x10_2m")
    ap.add_argument("--nenv", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--preloop", type=int, default=50)
    ap.add_argument("--agents", type=int, default=1, help="n_agents_modal of the layout")
    ap.add_argument("--checkpoints", default=None, help="directory of actor checkpoints, one per agent")
    ap.add_argument("--nfiltered", type=int, default=5)
    ap.add_argument("--modes", type=int, nargs=2, default=None, help="n_zernike_start_end")
    ap.add_argument("--gamma", type=float, default=1.0, help="centroid gain")
    ap.add_argument("--accumulate-from", type=int, default=0,
                    help="first frame of the moments (0: the reference's cov_cor, preloop included)")
    ap.add_argument("--seed", type=int, default=200)
    ap.add_argument("--save", default=None, help=".npz of the histories of environment 0")
    ap.add_argument("--psf-rec", action="store_true", help="reconstruct the long-exposure PSF of environment 0 (Vii)")
    ap.add_argument("--psf-rec-out", default=None, help=".npz for otftel, otf2 and psf of --psf-rec")
    ap.add_argument("--groot", action="store_true", help="the GROOT model's bandwidth + tomography covariance and PSF "
                    "beside ROKET's measured ones, environment 0 (groot.test_Cerr)")
    a = ap.parse_args(argv)
    from ao_marl_amd import roket
    from ao_marl_amd.env import VecAoEnv
    rl = dict(n_reverse_filtered_from_cmat=a.nfiltered)
    if a.modes is not None:
        rl["n_zernike_start_end"] = list(a.modes)
    # an agent layout needs the range of modes it is dealt over (--modes); the integrator alone needs no layout
    with_layout = a.modes is not None or a.checkpoints is not None
    env = VecAoEnv(a.params, a.nenv, rl, n_agents_modal=a.agents if with_layout else None, geo=True, frame_pipeline=False)
    env.set_sim_seed(a.seed)                         # error_budget_multiple_agents.py:291-292
    policy = None
    if a.checkpoints:
        from ao_marl_amd.sac import BatchedSAC
        sac = BatchedSAC(env.layout, dict(memory_size=16))
        files = sorted(f for f in os.listdir(a.checkpoints) if not f.startswith("."))
        if len(files) != env.layout.n_agents:
            raise SystemExit("--checkpoints: %d files for %d agents" % (len(files), env.layout.n_agents))
        for i, f in enumerate(files):
            sac.load_model(i, os.path.join(a.checkpoints, f))
        policy = sac.policy
    rk = roket.VecRoket(env, a.frames, a.preloop, policy=policy, gamma=a.gamma, accumulate_from=a.accumulate_from,
                        keep_envs=(0,) if a.save or a.psf_rec or a.groot else (), psf_ortho_envs=(0,) if a.psf_rec else ())
    res = rk.run()
    names = res["contributors"]
    cov, cor = res["cov"].mean(axis=0), res["cor"].mean(axis=0)
    print("\n%s, %d environments, %d frames (%d preloop), moments over %d frames" %
          (a.params, a.nenv, a.frames, a.preloop, res["frames"]))
    print("%-16s %14s %10s" % ("contributor", "variance", "share"))
    tot = float(np.trace(cov))
    for k, n in enumerate(names):
        print("%-16s %14.6e %9.1f%%" % (n, cov[k, k], 100.0 * cov[k, k] / tot if tot > 0 else 0.0))
    print("%-16s %14.6e   (sum of the diagonal)" % ("total", tot))
    print("%-16s %14.6e   (all pairs: variance of the sum)" % ("sum", float(cov.sum())))
    print("\ncorrelation (mean over environments)")
    print(" " * 16 + " ".join("%8s" % n[:8] for n in names))
    for k, n in enumerate(names):
        print("%-16s" % n + " ".join("%8.3f" % cor[k, l] for l in range(len(names))))
    k = res["rad2_per_um2"]
    fit = float(res["fitting"].mean())
    print("\nfitting (mean phase variance behind the geometric controller) %.6e um^2 = %.5f rad^2" % (fit, fit * k))
    budget = float(cov.sum()) * k + fit * k
    print("budget: variance of the sum %.5f rad^2 + fitting %.5f rad^2 = %.5f rad^2 -> exp(-.) = %.4f" %
          (float(cov.sum()) * k, fit * k, budget, float(np.exp(-budget))))
    print("closure: exp(-budget) - SR long exposure = %+.4f" % (float(np.exp(-budget)) - float(res["SR"].mean())))
    print("SR long exposure %.4f   SR2 = exp(-mean phase variance) %.4f" % (float(res["SR"].mean()), float(res["SR2"].mean())))
    print("centroid gain %.4f   centroid gain 2 %.4f" % (float(res["centroid_gain"].mean()), float(res["centroid_gain2"].mean())))
    if a.save:
        rk.save(a.save)
        print("histories of environment 0 -> %s" % a.save)
    if a.psf_rec:
        # a comparison, not a check: how closely a covariance of a few hundred frames explains the PSF is physics
        from ao_marl_amd import psf_rec
        with_zeta = policy is not None
        otftel, otf2, psf = psf_rec.psf_rec_vii(rk, 0, fitting=True, rl=with_zeta)
        bare = psf_rec.psf_rec_vii(rk, 0, fitting=False, rl=with_zeta)[2]
        print("PSF reconstruction (Vii), environment 0: Strehl %.4f with the fitting OTF, %.4f without   |   loop: SR long "
              "exposure %.4f, SR2 %.4f" % (float(psf.max()), float(bare.max()), float(res["SR"][0]), float(res["SR2"][0])))
        if a.psf_rec_out:
            np.savez(a.psf_rec_out, otftel=otftel, otf2=otf2, psf=psf, psf_without_fitting=bare)
            print("otftel, otf2, psf -> %s" % a.psf_rec_out)
    if a.groot:
        # groot.test_Cerr (:215-246) without its plots: how well the model fits this simulator is a result, not a check
        from ao_marl_amd import groot, psf_rec
        d, rec = psf_rec.from_source(rk)
        model = groot.GrootModel(rk)
        measured = psf_rec.covmodes_from(d, 0, contributors=["bandwidth", "tomography"])
        cerr = model.cerr()
        sr = lambda c: float(rec.reconstruct(c)["strehl"])                         # noqa: E731
        print("GROOT, environment 0 (variances in um^2, x %.4f for rad^2 at the target):" % k)
        print("  bandwidth + tomography   ROKET trace %.6e   model trace %.6e   ratio %.3f" %
              (np.trace(measured), np.trace(cerr), np.trace(cerr) / np.trace(measured)))
        print("  largest mode             ROKET %.6e   model %.6e" % (np.diag(measured).max(), np.diag(cerr).max()))
        print("  PSF of that covariance alone (no fitting): Strehl ROKET %.4f   model %.4f" % (sr(measured), sr(cerr)))
        full = model.psf(env=0, rec=rec)
        print("  model PSF (Cerr + measured noise + Calias, fitting OTF): Strehl %.4f   |   loop: SR long exposure %.4f" %
              (full["strehl"], float(res["SR"][0])))
        # the reference's Nact^-1 yields commands of unit-peak influence functions; this mirror's peak at unitpervolt
        u = model.stroke_scale
        if u is not None and u != 1.0:
            print("  the mirror's unitpervolt puts the model's Cerr a factor %.4g below the commands' volts^2 (GrootModel."
                  "stroke_scale); with cerr_scale = %.4g:" % (u, u))
            print("  bandwidth + tomography   model trace %.6e   ratio to ROKET %.3f   Strehl of that covariance alone %.4f" %
                  (np.trace(cerr) * u, np.trace(cerr) * u / np.trace(measured), sr(cerr * u)))
            print("  model PSF: Strehl %.4f" % model.psf(env=0, rec=rec, cerr_scale=u)["strehl"])
    return res


if __name__ == "__main__":
    main()
