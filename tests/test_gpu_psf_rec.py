"""PSF reconstruction on the device (csrc/aomarl_psfrec.hip through ao_marl_amd/psf_rec.py) against the float64
restatement (tests/psf_rec_reference.py).

Tolerances: the yardstick is float64; the allowance is 4 x the error of the SAME statement in float32 on the CPU
(ViiReconstructor(device="cpu", dtype=np.float32): NumPy complex64 transforms on the same inputs), measured by the test
at run time -- the project's convention for fp32 kernels checked against float64.  dphi and otf2 are
compared on the WHOLE mask, the psf relative to its peak.  Every test prints the device's error beside the CPU's."""
import ctypes as C

import numpy as np
import pytest

from tests import psf_rec_reference as pr
from tests.test_psf_rec import GOLDEN, tilt_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM = 1.65


def _errors(got, ref):
    """max |dphi| and |otf2| error over the whole mask, max |psf| error relative to the peak"""
    on = ref["mask"] != 0
    return (float(np.abs(got["dphi"] - ref["dphi"])[on].max()), float(np.abs(got["otf2"] - ref["otf2"])[on].max()),
            float(np.abs(got["psf"] - ref["psf"]).max() / ref["psf"].max()))


def _check(tag, gpu, f32, ref):
    eg, ec = _errors(gpu, ref), _errors(f32, ref)
    for name, g, c in zip(("dphi", "otf2", "psf/peak"), eg, ec):
        print("%s %-8s device %.3e   CPU float32 %.3e   allowance %.3e" % (tag, name, g, c, 4 * c))
    for name, g, c in zip(("dphi", "otf2", "psf/peak"), eg, ec):
        assert g <= 4 * c, (tag, name, g, c)
    off = ref["mask"] == 0
    assert not gpu["otf2"][off].any() and not gpu["dphi"][off].any()


def _third():
    """p = 40, N = 128, obstruction 0.2, 37 modes; a covariance of rank 24 from 24 frames: a third of its eigenvalues
    are zero or slightly negative"""
    s = pr.synthetic_system(40, 0.2, 6, 37, seed=5)
    y = np.random.default_rng(6).normal(size=(37, 24)) * 0.05
    s["cov"] = y.dot(y.T) / 24
    e = np.linalg.eigvalsh(s["cov"])
    assert (e < 1e-12 * e.max()).sum() == 13 and (e < 0).any()
    return s


@pytest.fixture(scope="module")
def cases():
    """name -> (reconstructor arguments, covmodes, float64 restatement); computed once, left unchanged"""
    out = {}
    with np.load(GOLDEN) as z:
        for n in ("A", "B"):
            c = pr.case(z, n)
            out[n] = ((c["spup"], (c["IF.data"], c["IF.indices"], c["IF.indptr"]), c["TT"], c["Btt"], c["tar_lambda"]),
                      pr.covmodes_of(c))
    s = _third()
    out["C"] = ((s["spup"], s["IF"], s["TT"], s["Btt"], LAM), s["cov"])
    for n, (args, cov) in list(out.items()):
        ref = pr.vii_f64(args[0], args[1], args[2], args[3], cov, args[4])
        assert 0.3 <= ref["psf"].max() <= 0.99, (n, ref["psf"].max())
        out[n] = (args, cov, ref)
    return out


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_native_against_float64(cases, name):
    """N = 64 and 128 (LDS passes of different depth), p = 24, 33, 40 (odd and even, no multiple of the wave size; 33 is
    no multiple of 4), 16 / 30 / 37 modes (no multiple of a batch), pixels under 16 influence functions and under none"""
    from ao_marl_amd import psf_rec
    args, cov, ref = cases[name]
    gpu = psf_rec.ViiReconstructor(*args, device=DEV).reconstruct(cov)
    f32 = psf_rec.ViiReconstructor(*args, device="cpu", dtype=np.float32).reconstruct(cov)
    assert gpu["psf"].dtype == np.float32 and gpu["psf"].shape == ref["psf"].shape
    _check("case %s" % name, gpu, f32, ref)


def test_determinism(cases):
    """one call of 37 modes and calls of 16 + 16 + 5 leave the same bits; so do a second run and a second finish"""
    import torch
    from ao_marl_amd import psf_rec
    args, cov, _ = cases["C"]
    rec = psf_rec.ViiReconstructor(*args, device=DEV)
    com, w = rec.modes_of(cov)
    assert com.shape[0] == 37
    rec.reset()
    rec.accumulate(com, w)
    one = rec.finish()
    again = rec.finish()
    rec.reset()
    for a, b in ((0, 16), (16, 32), (32, 37)):
        rec.accumulate(com[a:b], w[a:b])
    split = rec.finish()
    rec.reset()
    rec.accumulate(com, w)
    rerun = rec.finish()
    torch.cuda.synchronize()
    for k, name in enumerate(("dphi", "otf2", "psf")):
        assert torch.equal(one[k], again[k]), "finish twice: " + name
        assert torch.equal(one[k], split[k]), "16 + 16 + 5: " + name
        assert torch.equal(one[k], rerun[k]), "second run: " + name
    assert float(one[2].max()) > 0.3


def test_zero_tilt_and_refusal(cases):
    from ao_marl_amd import libaomarl as la
    from ao_marl_amd import psf_rec
    eps = float(np.finfo(np.float32).eps)
    # zero covariance: dphi is exactly zero, otf2 is the mask, the peak is 1 up to the last transform's round-off.
    # Every output of a radix-2 transform passes log2 N butterflies per dimension, each with one rounded sum and one
    # rounded twiddle product (<= 2 eps together) on data of one sign: 4 log2(N) eps; the float32 copy of otftel, the
    # division by the maximum and the scale 1 / npts add less than 8 eps more.
    args, _, ref = cases["A"]
    rec = psf_rec.ViiReconstructor(*args, device=DEV)
    r = rec.reconstruct(np.zeros((args[3].shape[1],) * 2))
    bound = (4 * np.log2(rec.N) + 8) * eps
    print("zero covariance: |psf.max() - 1| = %.3e, bound %.3e" % (abs(float(r["psf"].max()) - 1), bound))
    assert np.array_equal(r["otf2"], ref["mask"].astype(np.float32)) and not r["dphi"].any()
    assert abs(float(r["psf"].max()) - 1.0) <= bound
    # pure tilt against its closed form; allowance: 4 x the CPU float32 statement's error against the same closed form
    targs, tcov, want = tilt_case()
    gpu = psf_rec.ViiReconstructor(*targs, device=DEV)
    w = want(gpu.N)
    on = gpu.tel["mask"] != 0
    eg = float(np.abs(gpu.reconstruct(tcov)["dphi"] - w)[on].max())
    ec = float(np.abs(psf_rec.ViiReconstructor(*targs, device="cpu", dtype=np.float32).reconstruct(tcov)["dphi"] - w)[on].max())
    print("pure tilt dphi: device %.3e   CPU float32 %.3e   allowance %.3e   (largest value %.3e)" % (eg, ec, 4 * ec, w[on].max()))
    assert eg <= 4 * ec
    # N = 4096 is refused by the library, naming N
    d = la.PsfRecDesc()
    d.p, d.N, d.npts, d.nactu, d.ld_actu = 1024, 4096, 10, 5, 5
    ptr = C.c_void_p()
    with pytest.raises(la.AomarlError, match="N = 4096"):
        la.check(la.load().aomarl_psfrec_create(C.byref(d), C.byref(ptr)))
    assert not ptr.value


def test_10x10_end_to_end(tmp_path):
    """VecRoket on the 10x10 system -> psf_rec_vii on the device against the restatement on the saved file: p = 160,
    N = 512, 87 modes; with and without the run's own fitting PSF"""
    from ao_marl_amd import psf_rec, roket
    from ao_marl_amd.env import VecAoEnv
    env = VecAoEnv("production_sh_10x10_2m", 2, geo=True, frame_pipeline=False)
    rk = roket.VecRoket(env, 30, 5, keep_envs=(0, 1), psf_ortho_envs=(0, 1))
    rk.run(verbose=False)
    d, rec = psf_rec.from_source(rk)
    assert rec.device.startswith("cuda") and rec.N == 512 and rec.p == 160 and d["Btt"].shape[1] == 87
    plain = psf_rec.psf_rec_vii(rk, fitting=False, rec=rec)
    fitted = psf_rec.psf_rec_vii(rk, fitting=True, rec=rec)
    path = str(tmp_path / "budget.npz")
    rk.save(path)
    with np.load(path) as z:
        f = {k: z[k] for k in z.files}
    assert f["psfortho"].shape == (2, 512, 512) and float(f["tar_lambda"][0]) == float(env.supervisor.s.tar_lambda)
    csr = (f["IF.data"], f["IF.indices"], f["IF.indptr"])
    cpu32 = psf_rec.ViiReconstructor(f["spup"], csr, f["TT"], f["Btt"], float(f["tar_lambda"][0]), device="cpu",
                                     dtype=np.float32)
    for i, e in enumerate((0, 1)):
        cov = pr.covmodes_of(f, i)
        ref = pr.vii_f64(f["spup"], csr, f["TT"], f["Btt"], cov, float(f["tar_lambda"][0]))
        g = rec.reconstruct(cov)
        assert np.array_equal(g["otf2"], plain[i][1]) and np.array_equal(g["psf"], plain[i][2])
        c32 = cpu32.reconstruct(cov)
        _check("10x10 env %d" % e, g, c32, ref)
        # fitting: the restatement's last product with the OTF of the run's own psfortho
        fit = pr.fitting_otf_centred(f["psfortho"][i])
        want = pr.psf_with(fit, ref["otf2"], rec.npts)
        got32 = cpu32.psf_from(c32["otf2"], fit)
        eg = float(np.abs(fitted[i][2] - want).max() / want.max())
        ec = float(np.abs(got32 - want).max() / want.max())
        print("10x10 env %d fitted psf/peak device %.3e   CPU float32 %.3e   allowance %.3e   (Strehl %.4f, fitted %.4f)"
              % (e, eg, ec, 4 * ec, ref["psf"].max(), want.max()))
        assert eg <= 4 * ec
