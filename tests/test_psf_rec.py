"""PSF reconstruction from the ROKET covariance (ao_marl_amd/psf_rec.py; reference: guardians/gamora.py:24-171), CPU side:
the float64 restatement and the product's CPU statement against the reference's own outputs (tests/golden/
psf_rec_vii.npz, tools/gen_golden_psf_rec.py), the size rule, the covariance of a sum of contributors, two hand-worked
cases and the layout of the fitting PSF."""
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp

from tests import psf_rec_reference as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psf_rec_vii.npz")
TOL = 1e-9      # both sides float64, O(1) values, sums of <= 16384 terms: round-off ~1e-13; one mask pixel, a dropped
#                 tip-tilt term or a wrong eigenvector pairing shows above 1e-4


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        cases = {n: pr.case(z, n) for n in ("A", "B")}
    for n, c in cases.items():                       # precondition on the fixture: a Strehl that means something
        assert 0.3 <= float(c["psf"].max()) <= 0.99, (n, float(c["psf"].max()))
    return cases


def _close(got, want):
    return np.abs(got - want).max() <= TOL * np.abs(want).max()


def _csr(c):
    return (c["IF.data"], c["IF.indices"], c["IF.indptr"])


def test_restatement_against_the_reference(golden):
    for n, c in golden.items():
        r = pr.vii_f64(c["spup"], _csr(c), c["TT"], c["Btt"], pr.covmodes_of(c), c["tar_lambda"])
        for k in ("otftel", "otf2", "psf"):
            assert _close(r[k], c[k]), (n, k, np.abs(r[k] - c[k]).max() / np.abs(c[k]).max())
        # the reference's mask, pixel for pixel: otf2 is exp(.) > 0 exactly where the mask is 1
        assert np.array_equal(r["mask"] != 0, c["otf2"] != 0), n


def test_fft_size(golden):
    from ao_marl_amd import psf_rec
    for n, c in golden.items():
        assert psf_rec.fft_size(c["spup"].shape[0]) == c["otf2"].shape[0] == {"A": 64, "B": 128}[n]
    for p in (12, 16, 24, 32, 33, 160, 640):
        mradix = 2
        assert psf_rec.fft_size(p) == mradix ** int((np.log(2 * p) / np.log(mradix)) + 1), p


def test_cpu_statement_against_the_reference(golden):
    """the one-transform form of the first term against the reference's per-mode form"""
    from ao_marl_amd import psf_rec
    for n, c in golden.items():
        rec = psf_rec.ViiReconstructor(c["spup"], _csr(c), c["TT"], c["Btt"], c["tar_lambda"], device="cpu")
        r = rec.reconstruct(psf_rec.covmodes_from(c, 0))
        for k in ("otftel", "otf2", "psf"):
            assert _close(r[k], c[k]), (n, k, np.abs(r[k] - c[k]).max() / np.abs(c[k]).max())
        assert r["strehl"] == r["psf"].max()
        assert np.array_equal(rec.tel["mask"] != 0, c["otf2"] != 0), n
        both = rec.reconstruct(np.stack([psf_rec.covmodes_from(c, 0)] * 2))          # a batch of covariances
        assert both["psf"].shape == (2,) + c["psf"].shape and np.array_equal(both["psf"][1], r["psf"])


def _synthetic(rng, nenv=3, na=9, nm=7, nf=21):
    d = {k: rng.normal(size=(nenv, na, nf)) for k in pr.DEFAULT_SUM + ("zeta_com",)}
    d["P"] = rng.normal(size=(nm, na))
    d["envs"] = np.array([4, 1, 6][:nenv])
    return d


def test_covmodes_from(tmp_path):
    from ao_marl_amd import psf_rec, roket
    rng = np.random.default_rng(3)
    d = _synthetic(rng)

    def direct(i, names):
        y = d["P"].dot(sum(d[k][i] for k in names))
        return y.dot(y.T) / y.shape[1]

    assert np.allclose(psf_rec.covmodes_from(d, 1), direct(1, pr.DEFAULT_SUM), rtol=1e-12, atol=0)
    assert np.allclose(psf_rec.covmodes_from(d, 6, rl=True), direct(2, pr.DEFAULT_SUM + ("zeta_com",)), rtol=1e-12, atol=0)
    assert np.allclose(psf_rec.covmodes_from(d, 4, contributors=["bandwidth", "noise"]), direct(0, ("bandwidth", "noise")),
                       rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="environment 2"):
        psf_rec.covmodes_from(d, 2)
    # a source without histories is refused by name
    bare = {"P": d["P"], "envs": d["envs"]}
    with pytest.raises(ValueError, match="no kept histories.*'noise'"):
        psf_rec.covmodes_from(bare, 1)
    # the .npz VecRoket.save writes, spup / tar_lambda included
    na, nm, nsl, npts, kept, nf, pre = 9, 7, 12, 20, 3, 8, 2
    hist = {"x": [rng.normal(size=(7, kept, na)) for _ in range(nf)]}
    for k, w in (("com", na), ("slopes", nsl), ("wf_com", na), ("alias_meas", nsl), ("trunc_meas", nsl)):
        hist[k] = [rng.normal(size=(kept, w)) for _ in range(nf)]
    cal = types.SimpleNamespace(IF=sp.random(npts, na, density=0.4, random_state=1, format="csc"), P=d["P"],
                                Btt=rng.normal(size=(na, nm)), imat=rng.normal(size=(nsl, na)))
    res = dict(fitting=np.arange(8.), SR=np.arange(8.), SR2=None, cov=np.zeros((8, 6, 6)), cor=np.zeros((8, 6, 6)),
               centroid_gain=np.ones(8), centroid_gain2=np.ones(8))
    spup = np.ones((5, 4), dtype=np.float32)
    f = roket.npz_dict(hist, [2, 0], [7, 3], pre, res, cal, rng.normal(size=(na, nsl)), spup=spup, tar_lambda=1.65)
    assert np.array_equal(f["spup"], spup) and float(f["tar_lambda"][0]) == 1.65
    np.savez(str(tmp_path / "budget.npz"), **f)
    x = np.stack(hist["x"])[pre:]                                        # [frames][7][kept][nactu]
    err = sum(x[:, k, 0].T for k in (0, 1, 2, 3, 4, 5))                  # environment 3 is kept environment 0 (idx)
    y = d["P"].dot(err)
    assert np.allclose(psf_rec.covmodes_from(str(tmp_path / "budget.npz"), 3), y.dot(y.T) / y.shape[1], rtol=1e-12, atol=0)


def _disc(p, cobs=0.2):
    y, x = np.mgrid[:p, :p] - (p - 1) / 2.0
    r = np.hypot(x, y) / (p / 2.0)
    return ((r <= 1.0) & (r >= cobs)).astype(np.float64), x, y


def tilt_case(p=24, a=0.013, e=1.7, lam=1.65):
    """one mode m = a x over a centro-symmetric pupil with variance e: (reconstructor arguments, covmodes, dphi wanted
    as a function of the reconstructor's N)"""
    spup, x, y = _disc(p)
    lit = np.nonzero(spup)
    npts = lit[0].size
    IF = sp.csr_matrix((1, npts))
    TT = np.stack([x[lit], y[lit]], axis=1)
    Btt = np.array([[0.0], [a], [0.0]])

    def want(N):
        rho = np.arange(N)
        rho = np.where(rho < N // 2, rho, rho - N).astype(np.float64)
        return np.broadcast_to(e * a * a * rho[None, :] ** 2 * (2 * np.pi / lam) ** 2, (N, N))

    return (spup, IF, TT, Btt, lam), np.array([[e]]), want


def test_zero_covariance(golden):
    from ao_marl_amd import psf_rec
    c = golden["A"]
    rec = psf_rec.ViiReconstructor(c["spup"], _csr(c), c["TT"], c["Btt"], c["tar_lambda"], device="cpu")
    r = rec.reconstruct(np.zeros((c["Btt"].shape[1],) * 2))
    assert np.abs(r["otf2"] - rec.tel["mask"]).max() <= 1e-12
    assert abs(r["psf"].max() - 1.0) <= 1e-12                             # N^2 / npts makes the diffraction peak 1


def test_pure_tilt():
    """D(rho) = <(m(r) - m(r + rho))^2> = e a^2 rho_x^2 for m = a x: worked by hand, no restatement involved"""
    from ao_marl_amd import psf_rec
    args, cov, want = tilt_case()
    rec = psf_rec.ViiReconstructor(*args, device="cpu")
    r = rec.reconstruct(cov)
    w = want(rec.N)
    on = rec.tel["mask"] != 0
    assert on.sum() > 1000
    assert np.abs(r["dphi"] - w)[on].max() <= 1e-9 * w[on].max()


def test_fitting_convention(golden):
    """psfortho = the pupil's own diffraction PSF, laid out as VecRoket.save lays it out (zero frequency in the middle):
    its OTF is the telescope's, so fitting changes nothing"""
    from ao_marl_amd import psf_rec
    c = golden["A"]
    N = c["otf2"].shape[0]
    pup = np.zeros((N, N))
    pup[:24, :24] = c["spup"]
    d = {k: (v[None] if k in pr.DEFAULT_SUM else v) for k, v in c.items()}
    d["envs"] = np.array([5])
    d["psfortho"] = np.fft.fftshift(np.abs(np.fft.fft2(pup)) ** 2)[None]
    with_fit = psf_rec.psf_rec_vii(d, 5, fitting=True)
    without = psf_rec.psf_rec_vii(d, 5, fitting=False)
    assert _close(with_fit[2], without[2]) and _close(without[2], c["psf"])
    assert np.array_equal(with_fit[1], without[1])
    # the refusals, by name
    d["psfortho"] = d["psfortho"][:, :32, :32]
    with pytest.raises(ValueError, match="psfortho.*N = 64"):
        psf_rec.psf_rec_vii(d, 5, fitting=True)
    d.pop("psfortho")
    d["spup"] = c["spup"] * 0.5
    with pytest.raises(ValueError, match="spup is not binary"):
        psf_rec.psf_rec_vii(d, 5)
