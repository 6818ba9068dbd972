"""The GROOT covariance model (ao_marl_amd/groot.py; reference: guardians/groot.py, guardians/starlord.py), CPU side: the
float64 restatement (tests/groot_reference.py) and the product's CPU statement against the reference's own outputs
(tests/golden/groot.npz, tools/gen_golden_groot.py), the coupling matrix, symmetries, batching, refusals and the
stand-alone host program of the native path's host half."""
import os
import subprocess

import numpy as np
import pytest

from tests import groot_reference as gr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "groot.npz")
CSRC = os.path.join(os.path.dirname(HERE), "ao_marl_amd", "csrc")
TOL = 1e-9      # both sides float64; second differences of structure functions a few hundred times the result, projected
#                 through matrices of order <= 71: round-off ~1e-13.  A wrong x0, sign of an offset, weight of a Simpson
#                 offset or branch point shows above 1e-4.


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        out = {n: gr.case(z, n) for n in ("A", "B")}
        out["fn"] = {k: z[k] for k in z.files if k.startswith(("fn_", "nact_", "B_count_"))}
    return out


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _model(c, **kw):
    from ao_marl_amd import groot
    return groot.GrootModel(c, **kw)


def test_structure_functions(golden):
    """on a vector of separations that straddles every branch: r = 0, both sides of x = e^-3, of the table's end and of
    2 pi r / L0 = 4.71239 for three outer scales"""
    from ao_marl_amd import groot
    f = golden["fn"]
    r, x0 = f["fn_r"], float(f["fn_x0"])
    tabx, taby = groot.tabulate_ij0()
    assert tabx.shape == taby.shape == (10000,)
    assert np.array_equal(np.stack([tabx[::500], taby[::500]]), f["fn_tab_probe"])
    x = r * (np.pi / x0)
    assert (x < np.exp(-3.0)).sum() >= 3 and (x > tabx[-1]).sum() >= 2      # the series; beyond the table's end
    for mod in (groot, gr):
        assert _rel(mod.ij0t83(x), f["fn_ij0t83"]) <= TOL
        assert _rel(mod.dphi_highpass(r, x0), f["fn_dphi_highpass"]) <= TOL
        for i, L0 in enumerate(f["fn_L0"]):
            big = (2 * np.pi / L0) * r > 4.71239
            assert big.sum() >= 3 and (~big).sum() >= 3
            assert _rel(mod.rodconan(r, L0), f["fn_rodconan"][i]) <= TOL
            assert _rel(mod.dphi_lowpass(r, x0, L0), f["fn_dphi_lowpass"][i]) <= TOL
        assert mod.dphi_highpass(np.zeros(1), x0)[0] == 0 and mod.rodconan(np.zeros(1), 25.)[0] == 0
    assert np.array_equal(groot.ij0t83(np.array([tabx[-1] * 2, 1e9])), taby[[-1, -1]])   # clamped to the last entry
    assert np.array_equal(groot.simpson_coeff(5), [1, 4, 2, 4, 1]) and np.array_equal(groot.simpson_coeff(1), [1])


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_against_the_reference(golden, name):
    c = golden[name]
    assert _rel(gr.cerr(c, modal=True), c["out_cerr_modal"]) <= TOL
    assert _rel(gr.calias(c, slopes_space=True, npts=3), c["out_calias_slopes_3"]) <= TOL
    assert _rel(gr.calias(c, slopes_space=True, npts=5), c["out_calias_slopes_5"]) <= TOL
    assert _rel(gr.calias(c), c["out_calias_modal_3"]) <= TOL
    assert _rel(gr.dcmm(c), c["out_dcmm"]) <= TOL
    ws, wd = np.asarray(c["_Param_atmos__windspeed"]) * 0.5, np.asarray(c["_Param_atmos__winddir"]) + 30.
    assert _rel(gr.dcmm(c, ws=ws, wd=wd, dk=2), c["out_dcmm_dk2"]) <= TOL
    _cerr_blocks("restatement " + name, gr.cerr(c, modal=False), c)


def _cerr_blocks(tag, got, c):
    """the pzt block to 1e-9; the 2 x 2 tip-tilt block to the float32 level of the reference's pzt2tt: 4 x the gap that
    opens when that matrix is made in float64 instead (measured here, printed beside the error); the cross terms zero"""
    want = c["out_cerr_actu"]
    assert _rel(got[:-2, :-2], want[:-2, :-2]) <= TOL, tag
    gap = _rel(gr.cerr(c, modal=False, pzt2tt=gr.pzt2tt_f64(c))[-2:, -2:], want[-2:, -2:])
    err = _rel(got[-2:, -2:], want[-2:, -2:])
    print("%s tip-tilt block: error %.3e, float64-pzt2tt gap %.3e, allowance %.3e (largest value %.3e)" %
          (tag, err, gap, 4 * gap, np.abs(want[-2:, -2:]).max()))
    assert 1e-9 < gap < 1e-5, gap                       # float32 round-off, as the reference has it
    assert err <= 4 * gap, tag
    assert not got[:-2, -2:].any() and not got[-2:, :-2].any() and not want[:-2, -2:].any()


@pytest.mark.parametrize("name", ["A", "B"])
def test_cpu_statement_against_the_reference(golden, name):
    """the telescoped, collapsed and pre-composed forms against the reference's term-by-term ones"""
    from ao_marl_amd import psf_rec
    c = golden[name]
    m = _model(c)
    assert m.device == "cpu" and m.na == {"A": 45, "B": 69}[name] and m.nsub == {"A": 24, "B": 44}[name]
    assert _rel(m.cerr(), c["out_cerr_modal"]) <= TOL
    _cerr_blocks("statement " + name, m.cerr(modal=False), c)
    assert _rel(m.calias(slopes_space=True, npts=3), c["out_calias_slopes_3"]) <= TOL
    assert _rel(m.calias(slopes_space=True, npts=5), c["out_calias_slopes_5"]) <= TOL
    assert _rel(m.calias(), c["out_calias_modal_3"]) <= TOL
    assert _rel(m.dcmm(), c["out_dcmm"]) <= TOL
    assert _rel(m.dcmm(ws=m.speed * 0.5, wd=m.winddir + 30., dk=2), c["out_dcmm_dk2"]) <= TOL
    assert _rel(m.ca_gendron(), c["out_ca_gendron"]) <= TOL
    assert _rel(m.cn(model="model"), c["out_cn_model"]) <= TOL
    otf_fit, psf_fit = m.otf_fitting(psf_rec.telescope_otf(c["spup"])["otftel"])
    assert _rel(otf_fit, c["out_otf_fit"]) <= TOL and _rel(psf_fit, c["out_psf_fit"]) <= TOL
    assert 0.05 < psf_fit.max() < 1.0


def test_every_branch_is_taken_on_case_b(golden):
    """a condition on the fixture, not a measurement: Cerr, Calias and dCmm of case B evaluate both branches of rodconan
    and both of Ij0t83, in the restatement and in the product's statement, as the reference did when the golden was made"""
    from ao_marl_amd import groot
    c = golden["B"]
    gr.reset_counts()
    gr.cerr(c)
    gr.calias(c, slopes_space=True)
    gr.dcmm(c)
    for k in groot.branch_counts:
        groot.branch_counts[k] = 0
    m = _model(c)
    m.cerr()
    m.calias(slopes_space=True)
    m.dcmm()
    print("restatement", gr.COUNTS, "statement", groot.branch_counts)
    for k in gr.COUNTS:
        assert gr.COUNTS[k] > 0 and groot.branch_counts[k] > 0 and int(golden["fn"]["B_count_" + k]) > 0, k


def test_nact_equals_the_reference(golden):
    import scipy.sparse as sp
    from ao_marl_amd import modal
    f = golden["fn"]
    for tag, n in (("10x10", 88), ("40x40", 1284)):
        got = modal.nact_geom(f["nact_%s_i1" % tag], f["nact_%s_j1" % tag], float(f["nact_%s_pitch" % tag]),
                              float(f["nact_%s_coupling" % tag]), int(f["nact_%s_dim" % tag]))
        if tag == "10x10":
            want = f["nact_10x10_dense"]
        else:
            want = sp.csr_matrix((f["nact_40x40_data"], f["nact_40x40_indices"], f["nact_40x40_indptr"]), shape=(n, n)).toarray()
        assert got.shape == (n, n) and got.dtype == np.float32 and np.array_equal(got, want), tag
    for name in ("A", "B"):                                # the synthetic lattices
        c = golden[name]
        got = modal.nact_geom(c["lattice_i1"], c["lattice_j1"], float(c["lattice_pitch"]), 0.2, int(c["lattice_dim"]))
        assert np.array_equal(got.astype(np.float64), c["Nact"]), name
    with pytest.raises(ValueError, match="leaves the 40 x 40 support"):
        modal.nact_geom([8, 24, 36], [8, 8, 8], 8, 0.2, 40)
    with pytest.raises(ValueError, match="different pixels"):
        modal.nact_geom([8, 8], [8, 8], 8, 0.2, 40)


def test_symmetries_and_batches(golden):
    c = golden["B"]
    m = _model(c)
    ce, ca, dc = m.cerr(), m.calias(slopes_space=True), m.dcmm()
    assert np.abs(ce - ce.T).max() <= 1e-12 * np.abs(ce).max()
    assert np.abs(ca - ca.T).max() <= 1e-12 * np.abs(ca).max()         # every offset comes with its mirror image
    assert np.abs(dc + dc.T).max() <= 1e-12 * np.abs(dc).max() and np.abs(dc).max() > 0
    ns = m.nsub
    assert not ca[:ns, ns:].any() and not dc[ns:, :ns].any()
    # a batch over every override equals the single calls, which equal the restatement
    speed = np.array([[0.4, 20., 15.], [5., 5., 5.], [12., 0.5, 30.]])
    H = np.array([[0., 4000., 10000.], [0., 1000., 2000.], [500., 8000., 16000.]])
    theta = np.array([[0.1, -1.2, 3.0], [0., 0., 0.], [2., 1., -3.]])
    L0 = np.array([[2., 1e5, 25.], [25., 25., 25.], [1e5, 3., 50.]])
    r0, gain = np.array([0.12, 0.2, 0.08]), np.array([0.4, 0.3, 0.7])
    both = m.cerr(speed=speed, H=H, theta=theta, r0=r0, L0=L0, gain=gain)
    assert both.shape == (3, m.nm, m.nm)
    for b in range(3):
        one = m.cerr(speed=speed[b], H=H[b], theta=theta[b], r0=r0[b], L0=L0[b], gain=gain[b])
        assert one.shape == (m.nm, m.nm) and np.array_equal(one, both[b]), b
        want = gr.cerr(c, speed=speed[b], H=H[b], theta=theta[b], r0=r0[b], L0=L0[b], gain=gain[b])
        assert _rel(one, want) <= TOL, b
    some = m.cerr(modal=False, r0=r0)                                   # one override batched, the rest the file's
    assert some.shape == (3, m.nactu, m.nactu) and np.array_equal(some[0], m.cerr(modal=False, r0=0.12))
    d2 = m.dcmm(ws=speed[:2], wd=np.array([[10., -75., 200.], [0., 90., 180.]]))
    assert d2.shape == (2, 2 * ns, 2 * ns) and np.array_equal(d2[0], dc)
    # the same statement with the device's rounding points stays at the float32 level
    m32 = _model(c, dtype=np.float32)
    assert m32.cerr().dtype == np.float32 and _rel(m32.cerr(), ce) < 1e-4


def test_refusals(golden):
    from ao_marl_amd import groot
    c = golden["A"]
    m = _model(c)
    for npts in (2, 4, 0):
        with pytest.raises(ValueError, match="npts = %d.*simpson_coeff" % npts):
            m.calias(npts=npts)
    for k in ("Nact", "dm.xpos", "_Param_atmos__windspeed", "_Param_controller__gain"):
        with pytest.raises(ValueError, match="lacks %r" % k):
            groot.GrootModel({a: v for a, v in c.items() if a != k})
    with pytest.raises(ValueError, match="speed has shape \\(3,\\): 2 layers"):
        m.cerr(speed=[1., 2., 3.])
    with pytest.raises(ValueError, match="L0 has shape"):
        m.cerr(L0=25.)
    with pytest.raises(ValueError, match="disagree on the batch size"):
        m.cerr(speed=np.ones((2, 2)), r0=np.ones(3))
    bad = dict(c)
    bad["_Param_atmos__L0"] = np.array([25., 25., 25.])
    with pytest.raises(ValueError, match="_Param_atmos__L0 has 3 entries.*nscreens is 2"):
        groot.GrootModel(bad)
    bad = dict(c)
    bad["Nact"] = np.triu(c["Nact"])
    with pytest.raises(ValueError, match="Nact is not symmetric"):
        groot.GrootModel(bad)
    with pytest.raises(ValueError, match="model = 'guess'"):
        m.cn(model="guess")
    with pytest.raises(ValueError, match="otftel is \\(8, 8\\)"):
        m.otf_fitting(np.ones((8, 8)))


def test_npz_dict_writes_what_the_model_reads(golden, tmp_path):
    """roket.npz_dict with the new keyword arguments -> a file GrootModel reads; without them the file is as before"""
    import types
    import scipy.sparse as sp
    from ao_marl_amd import groot, roket
    c = golden["A"]
    na, nsl, kept, nf = c["P"].shape[1], c["R"].shape[1], 1, 4
    rng = np.random.default_rng(1)
    hist = {"x": [rng.normal(size=(7, kept, na)) for _ in range(nf)]}
    for k, w in (("com", na), ("slopes", nsl), ("wf_com", na), ("alias_meas", nsl), ("trunc_meas", nsl)):
        hist[k] = [rng.normal(size=(kept, w)) for _ in range(nf)]
    IF = sp.csr_matrix((c["IF.data"], c["IF.indices"], c["IF.indptr"]))
    cal = types.SimpleNamespace(IF=sp.hstack([IF.T, sp.csr_matrix(c["TT"])], format="csc"), P=c["P"], Btt=c["Btt"],
                                imat=rng.normal(size=(nsl, na)))
    res = dict(fitting=np.zeros(1), SR=np.zeros(1), SR2=None, cov=np.zeros((1, 6, 6)), cor=np.zeros((1, 6, 6)),
               centroid_gain=np.ones(1), centroid_gain2=np.ones(1))
    plain = roket.npz_dict(hist, [0], [0], 1, res, cal, c["R"], spup=c["spup"], tar_lambda=1.65)
    assert "Nact" not in plain and not any(k.startswith("_Param_") for k in plain)
    with pytest.raises(ValueError, match="lacks 'Nact'"):
        groot.GrootModel(plain)
    params = {k: v for k, v in c.items() if k.startswith("_Param_") and k != "_Param_target__Lambda"}
    full = roket.npz_dict(hist, [0], [0], 1, res, cal, c["R"], spup=c["spup"], tar_lambda=1.65, nact=c["Nact"],
                          dm_xpos=c["dm.xpos"], dm_ypos=c["dm.ypos"], params=params)
    assert full["Nact"].dtype == np.float32 and set(plain) < set(full)
    with pytest.raises(ValueError, match="params key 'gain'"):
        roket.npz_dict(hist, [0], [0], 1, res, cal, c["R"], params={"gain": 0.4})
    path = str(tmp_path / "budget.npz")
    np.savez(path, **full)
    m = groot.GrootModel(path)
    # R goes through the file's float32
    assert _rel(m.cerr(), c["out_cerr_modal"]) <= TOL and _rel(m.calias(slopes_space=True), c["out_calias_slopes_3"]) <= TOL
    assert _rel(m.cn(model="data"), _cn_data(full)) <= 1e-12


def _cn_data(d):
    N = np.asarray(d["noise"][0], dtype=np.float64)
    P = np.asarray(d["P"], dtype=np.float64)
    return P.dot(N.dot(N.T) / N.shape[1]).dot(P.T)


def _file_of_system(name, seed=5):
    """a mapping GrootModel reads, from a production system's own geometry (un-calibrated: all actuators; P, Btt, R and
    the influence functions are random, of the right shapes) -- with the sensor's own list of valid sub-apertures"""
    import scipy.sparse as sp
    from ao_marl_amd import modal, params
    from tests import helpers
    sysm, s = helpers.uncalibrated(name)
    ps, dm, w = params.builtin(name), s.dms[0], sysm.wfss[0]
    rng = np.random.default_rng(seed)
    na, nsub, npts = dm.ntotact, s.nslope // 2, 50
    Q, _ = np.linalg.qr(rng.normal(size=(na + 2, na - 1)))
    IF = sp.random(na, npts, density=0.2, random_state=seed, format="csr", dtype=np.float32)
    a = ps.p_atmos
    d = {"P": np.linalg.pinv(Q), "Btt": Q, "R": rng.normal(size=(na + 2, 2 * nsub)), "IF.data": IF.data, "IF.indices": IF.indices,
         "IF.indptr": IF.indptr, "TT": rng.normal(size=(npts, 2)).astype(np.float32), "tar_lambda": np.array([s.tar_lambda]),
         "Nact": modal.nact_geom(dm.i1, dm.j1, dm.pitch, ps.p_dms[0].coupling, dm.n2 - dm.n1 + 1), "dm.xpos": dm.xpos,
         "dm.ypos": dm.ypos, "_Param_atmos__r0": a.r0, "_Param_atmos__alt": np.asarray(a.alt), "_Param_atmos__L0": np.asarray(a.L0),
         "_Param_atmos__windspeed": np.asarray(a.windspeed), "_Param_atmos__winddir": np.asarray(a.winddir),
         "_Param_atmos__frac": np.asarray(a.frac) / np.sum(a.frac), "_Param_atmos__nscreens": a.nscreens,
         "_Param_loop__ittime": ps.p_loop.ittime, "_Param_controller__gain": ps.p_controllers[0].gain,
         "_Param_wfs__xpos": np.array([0.]), "_Param_wfs__ypos": np.array([0.]), "_Param_wfs__Lambda": np.array([s.wfs_lambda]),
         "_Param_wfs__nxsub": np.array([s.nxsub]), "_Param_wfs__npix": np.array([s.npix]), "_Param_tel__diam": ps.p_tel.diam,
         "_Param_tel__cobs": ps.p_tel.cobs, "_Param_geom__pupdiam": sysm.geom.pupdiam,
         "_Param_dm__nact": np.array([p.nact for p in ps.p_dms]),
         "_Param_dm__unitpervolt": np.array([p.unitpervolt for p in ps.p_dms])}
    own = {"_Param_wfs___validsubsx": np.asarray(s.validsubsx), "_Param_wfs___validsubsy": np.asarray(s.validsubsy)}
    return d, own, sysm, w


def test_the_sensors_own_sub_apertures():
    """the 10x10 system: the reference's radial rule finds 60 of its 64 sub-apertures, so a file without the sensor's
    list is refused by name; with it the sub-aperture corners are the sensor's own pixel positions (x from x, y from y),
    and Gendron's stencil couples every sub-aperture to its neighbours along the slope's own axis, in R's order"""
    from ao_marl_amd import groot
    d, own, sysm, w = _file_of_system("production_sh_10x10_2m")
    with pytest.raises(ValueError, match="60 valid sub-apertures.*___validsubsx.*R has 128 slopes"):
        groot.GrootModel(d)
    m = groot.GrootModel(dict(d, **own))
    assert m.nsub == 64 and abs(m.stroke_scale - 1e4) < 1e-6
    pix = m.diam / sysm.geom.pupdiam
    # validpuppix: the corner of the sub-aperture on the padded pupil (2 pixels of margin), the pupil centred on pupdiam / 2
    assert np.allclose(m.xsub, (np.asarray(w.validpuppixx) - 2 - sysm.geom.pupdiam / 2) * pix, rtol=0, atol=1e-12)
    assert np.allclose(m.ysub, (np.asarray(w.validpuppixy) - 2 - sysm.geom.pupdiam / 2) * pix, rtol=0, atol=1e-12)
    assert len(set(zip(m.xsub, m.ysub))) == 64 and np.ptp(m.xsub) == np.ptp(m.ysub) == 9 * m.dsub
    # Gendron's stencil from the positions alone: 1 on itself, -1/2 on the two neighbours along x (X slopes) / y (Y slopes)
    ns, dd = m.nsub, m.dsub
    dx, dy = m.xsub[None, :] - m.xsub[:, None], m.ysub[None, :] - m.ysub[:, None]
    near = lambda a, b: (np.abs(np.abs(a) - dd) < 1e-9) & (np.abs(b) < 1e-9)        # noqa: E731
    S = np.zeros((2 * ns, 2 * ns))
    S[:ns, :ns] = np.identity(ns) - 0.5 * near(dx, dy)
    S[ns:, ns:] = np.identity(ns) - 0.5 * near(dy, dx)
    assert near(dx, dy).sum() > 100 and not np.array_equal(near(dx, dy), near(dy, dx))
    step = m.diam / (m.dm_nact - 1)
    r0 = m.r0 * (m.lam_tar / 0.5) ** (6. / 5.)
    scale = 0.23 * (step / r0) ** (5 / 3.) * (m.lam_tar * 1e-6 / (2 * np.pi * step)) ** 2 * gr.RASC ** 2
    want = m.R.dot(S * scale).dot(m.R.T)
    assert _rel(m.ca_gendron(modal=False), want) <= 1e-12
    assert _rel(m.ca_gendron(), m.P.dot(want).dot(m.P.T)) <= 1e-12
    # the aliasing model on the same list against the restatement, which takes the list in its own way
    assert _rel(m.calias(slopes_space=True), gr.calias(dict(d, **own), slopes_space=True)) <= TOL
    # cerr_scale: the sum as the reference has it, and with Cerr in the commands' unit
    f = dict(d, **own)
    f["noise"] = np.random.default_rng(1).normal(size=(m.nactu, 6))
    m = groot.GrootModel(f)
    assert _rel(m.cee(cerr_scale=m.stroke_scale) - m.cee(), (m.stroke_scale - 1) * m.cerr()) <= 1e-9


def test_host_check_builds_and_passes(tmp_path):
    """groot_host_check.cpp under the address and undefined-behaviour sanitizers: the validators' refusals, the tap lists
    against the reference's loops, the scalar functions at r = 0 and across their branch points"""
    exe = str(tmp_path / "groot_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "groot_host_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "groot_host_check: ok"
