"""ROKET error breakdown (ao_marl_amd/roket.py, csrc/aomarl_roket.hip; reference: guardians/roket_generalized_rl.py).
CPU: the covariance table from moment sums, the float64 checker on a hand-worked case, the .npz layout, the refusals.
GPU: the native filter bank against that checker, its determinism and its structural zeros; VecRoket: the loop left
untouched bit for bit, the breakdown against its restatement over the CPU oracle, with a policy, on a noisy sensor."""
import numpy as np
import pytest

from tests import helpers
from tests import roket_reference as rr

NAME = "production_sh_10x10_2m"


# ------------------------------------------------------------------------------------------------------ CPU
def test_cov_cor_from_moments_equals_cov_cor_of_histories():
    """C1: cov / cor assembled from S1 / S2 equal the reference's cov_cor applied to whole histories."""
    from ao_marl_amd import roket
    rng = np.random.default_rng(0)
    n, na, nm = 57, 11, 9
    P = rng.normal(size=(nm, na))
    hist = {k: rng.normal(size=(n, na)) * (i + 1) + 0.3 * i for i, k in enumerate(rr.NAMES)}
    hist["bp"] = hist["noise"] * 0.5 + hist["bp"] * 0.1            # some correlation
    for with_zeta in (True, False):
        for start in (0, 20):
            S1, S2, frames = rr.moments(hist, P, start)
            assert frames == n - start
            cov, cor, var = roket.cov_cor_moments(S1, S2, frames, with_zeta)
            wcov, wcor = rr.cov_cor(hist, P, with_zeta, start)
            assert cov.shape == ((7, 7) if with_zeta else (6, 6))
            assert np.abs(cov - wcov).max() < 1e-11 * np.abs(wcov).max()
            assert np.abs(cor - wcor).max() < 1e-11
            assert np.allclose(np.diag(cor), 1.0)
            # the per-mode variances are what the table sums
            y = P.dot(hist["trunc"][start:].T)
            assert np.abs(var[1, 1] - y.var(axis=1)).max() < 1e-11 * y.var(axis=1).max()
    # a contributor that is identically zero: its row of cor stays zero, as in the reference
    hist["tomo"] = np.zeros((n, na))
    S1, S2, frames = rr.moments(hist, P)
    cov, cor, _ = roket.cov_cor_moments(S1, S2, frames)
    assert (cov[5] == 0).all() and (cor[5] == 0).all() and (cor[:, 5] == 0).all()
    with pytest.raises(ValueError):
        roket.cov_cor_moments(S1, S2, 0)


@pytest.mark.parametrize("delay", [1, 2])
def test_filter_bank_f64_on_a_hand_worked_case(delay):
    """C2: three actuators, P = Btt = I (mode 0 filtered, modes 1 and 2 the tip-tilt pair), RD = diag(1, 1/2, 1/4),
    g = 1/2, gamma = 1, so gRD = diag(1/2, 1/4, 1/8); constant inputs.  Every value below is worked out by hand."""
    n = 6
    one = np.ones((n, 3))
    B = one * [3.0, 4.0, 5.0]
    G = one * [3.0, 4.0, 6.0]
    h = rr.filter_bank_f64(derr=2 * one, E=one, F=0.5 * one, ageom=2 * one, B=B, G=G, rl_com=4 * one,
                           RD=np.diag([1.0, 0.5, 0.25]), P=np.eye(3), Btt=np.eye(3), g=0.5, gamma=1.0, nfiltered=1,
                           delay=delay)
    assert (h["noise_buf"] == 1).all() and (h["trunc_buf"] == 0.5).all()
    assert (h["H_com"] == [3, 0, 0]).all() and (h["mod_com"] == [0, 4, 5]).all() and (h["wf_com"] == [0, 4, 6]).all()
    assert (h["tomo_buf"] == [0, 0, -1]).all()
    if delay == 1:
        # x[t] = x[t-1] - gRD x[t-1] + g * 1
        assert (h["noise"][:3] == [[0, 0, 0], [0.5, 0.5, 0.5], [0.75, 0.875, 0.9375]]).all()
        # the same filter on g * 0.5: half the noise contributor
        assert (h["trunc"] == 0.5 * h["noise"]).all()
        # gamma g ageom = 1: twice the noise contributor;  rl_com = 4 (no gain): eight times
        assert (h["alias"] == 2 * h["noise"]).all() and (h["zeta"] == 8 * h["noise"]).all()
        # bandwidth: -C[0] = -mod_com[0] undelayed, then C = 0 and the filter decays it
        assert (h["bp"][:2] == [[0, -4, -5], [0, -3, -4.375]]).all()
        # tomography: -gRD tomo_buf[t-1] = +1/8 on the last actuator from frame 1 on
        assert (h["tomo"][:3] == [[0, 0, 0], [0, 0, 0.125], [0, 0, 0.234375]]).all()
    else:
        # x[t] = x[t-1] - gRD x[t-2] + g * 1 from frame 2 on
        want = [[0, 0, 0], [0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1], [1.25, 1.375, 1.4375]]
        assert (h["noise"][:5] == want).all()
        assert (h["zeta"] == 8 * h["noise"]).all()
        # bp[1] = bp[0] - gRD bp[-1] - 0 = bp[0];  bp[2] = bp[1] - gRD bp[0]
        assert (h["bp"][:3] == [[0, -4, -5], [0, -4, -5], [0, -3, -4.375]]).all()
        assert (h["tomo"][:4] == [[0, 0, 0], [0, 0, 0], [0, 0, 0.125], [0, 0, 0.25]]).all()
    # without G tomography vanishes, without a policy zeta does
    h0 = rr.filter_bank_f64(2 * one, one, 0.5 * one, 2 * one, B, None, None, np.diag([1.0, 0.5, 0.25]), np.eye(3),
                            np.eye(3), 0.5, 1.0, 1, delay)
    assert (h0["tomo"] == 0).all() and (h0["zeta"] == 0).all() and (h0["noise"] == h["noise"]).all()


# ------------------------------------------------------------------------------------------------------ GPU
N_FRAMES, N_ENV, N_FILT = 40, 3, 5
IN_NAMES = ("derr", "E", "F", "ageom", "B", "G", "rl_com")
_bank_case = {}


def _case():
    """Inputs of the bank tests and the float64 / float32 NumPy recursions on them, computed once."""
    if _bank_case:
        return _bank_case
    _, s, cal = helpers.calibrated(NAME)
    rng = np.random.default_rng(11)
    na, nm = s.nactu, cal.P.shape[0]
    Q, _ = np.linalg.qr(rng.normal(size=(na, 60)))
    c = _bank_case
    c["P"], c["Btt"] = np.asarray(cal.P, dtype=np.float32), np.asarray(cal.Btt, dtype=np.float32)
    c["RD"] = (Q @ Q.T).astype(np.float32)                    # eigenvalues 0 and 1: stable with g = 0.4
    c["g"], c["gamma"] = 0.4, 1.0
    c["na"], c["nm"] = na, nm
    c["in"] = {k: rng.normal(size=(N_FRAMES, N_ENV, na)).astype(np.float32) for k in IN_NAMES}
    c["scale"] = max(float(np.abs(v).max()) for v in c["in"].values())
    for delay in (1, 2):
        for with_g in (True, False):
            for dt in (np.float64, np.float32):
                out = []
                for e in range(N_ENV):
                    a = {k: v[:, e] for k, v in c["in"].items()}
                    out.append(rr.filter_bank_f64(a["derr"], a["E"], a["F"], a["ageom"], a["B"],
                                                  a["G"] if with_g else None, a["rl_com"], c["RD"], c["P"], c["Btt"],
                                                  c["g"], c["gamma"], N_FILT, delay, dtype=dt))
                c[(delay, with_g, dt)] = out
    return c


def _moments_f32(hist, P):
    """The bank's arithmetic in NumPy: y = P x in float32, the sums in float64."""
    y = [np.asarray(P, np.float32).dot(np.asarray(hist[k], np.float32).T).astype(np.float64) for k in rr.NAMES]
    S1 = np.stack([v.sum(axis=1) for v in y])
    S2 = np.stack([(y[k] * y[l]).sum(axis=1) for k in range(7) for l in range(k, 7)])
    return S1, S2


def _run_bank(delay, with_g):
    """-> (x [frames][7][nenv][nactu], bufs [frames][4][nenv][nactu], S1, S2, nframes) as NumPy arrays"""
    import torch
    from ao_marl_amd import roket
    c = _case()
    ld = (c["na"] + 3) // 4 * 4 + 4                           # a row stride that is not the row length
    bank = roket.RoketBank(N_ENV, c["RD"], c["P"], c["Btt"], c["g"], c["gamma"], N_FILT, delay, ld_actu=ld)
    dev = {}
    for k, v in c["in"].items():
        t = torch.full((N_FRAMES, N_ENV, ld), float("nan"), dtype=torch.float32, device="cuda:0")   # pads must not be read
        t[:, :, :c["na"]] = torch.from_numpy(v).to("cuda:0")
        dev[k] = t
    xs, bs = [], []
    for t in range(N_FRAMES):
        a = {k: v[t] for k, v in dev.items()}
        bank.step(a["derr"], a["E"], a["F"], a["ageom"], a["B"], a["G"] if with_g else None, a["rl_com"])
        x, b = bank.history()
        xs.append(x.cpu().numpy())
        bs.append(b.cpu().numpy())
    S1, S2, n = bank.moments()
    return np.stack(xs), np.stack(bs), S1, S2, n


@pytest.mark.gpu
@pytest.mark.parametrize("with_g", [True, False])
@pytest.mark.parametrize("delay", [1, 2])
def test_native_bank_matches_the_float64_recursion(delay, with_g):
    """G1.  Bound per contributor: 8 x the error of the same NumPy recursion run in float32 (the GEMM's summation
    order differs from NumPy's) + 1e-6 of the input scale.  For the moments the scale of that floor is the size of
    the sums themselves: frames x max|y| for S1, frames x max|y|^2 for S2."""
    c = _case()
    x, bufs, S1, S2, n = _run_bank(delay, with_g)
    assert n == N_FRAMES and np.isfinite(x).all() and np.isfinite(S1).all() and np.isfinite(S2).all()
    ymax = 0.0
    for e in range(N_ENV):
        h64, h32 = c[(delay, with_g, np.float64)][e], c[(delay, with_g, np.float32)][e]
        for k, name in enumerate(rr.NAMES):
            ref_err = float(np.abs(h32[name].astype(np.float64) - h64[name]).max())
            err = float(np.abs(x[:, k, e] - h64[name]).max())
            bound = 8 * ref_err + 1e-6 * c["scale"]
            print("delay %d G %d env %d %-6s: |hip - f64| = %.3e, |np32 - f64| = %.3e, ratio %.2f, max|x| = %.3g" %
                  (delay, with_g, e, name, err, ref_err, err / max(ref_err, 1e-30), np.abs(h64[name]).max()))
            assert err <= bound, (name, e, err, bound)
        for k, name in enumerate(("noise_buf", "trunc_buf", "tomo_buf", "mod_com")):
            ref_err = float(np.abs(h32[name].astype(np.float64) - h64[name]).max())
            err = float(np.abs(bufs[:, k, e] - h64[name]).max())
            assert err <= 8 * ref_err + 1e-6 * c["scale"], (name, e, err, ref_err)
        if not with_g:
            assert (x[:, 5, e] == 0).all() and (bufs[:, 2, e] == 0).all()
        w1, w2, _ = rr.moments(h64, c["P"])
        f1, f2 = _moments_f32(h32, c["P"])
        ymax = max(float(np.abs(np.asarray(c["P"], np.float64).dot(h64[k].T)).max()) for k in rr.NAMES)
        e1, e2 = np.abs(S1[e] - w1).max(), np.abs(S2[e] - w2).max()
        r1, r2 = np.abs(f1 - w1).max(), np.abs(f2 - w2).max()
        print("delay %d G %d env %d moments: S1 %.3e (np32 %.3e), S2 %.3e (np32 %.3e)" % (delay, with_g, e, e1, r1, e2, r2))
        assert e1 <= 8 * r1 + 1e-6 * N_FRAMES * ymax, (e, e1, r1)
        assert e2 <= 8 * r2 + 1e-6 * N_FRAMES * ymax * ymax, (e, e2, r2)


@pytest.mark.gpu
def test_native_bank_is_deterministic():
    """G2: two runs give the same bits, histories and moments."""
    a = _run_bank(2, True)
    b = _run_bank(2, True)
    for u, v in zip(a[:4], b[:4]):
        assert np.array_equal(u, v)
    assert a[4] == b[4]


@pytest.mark.gpu
def test_native_bank_structural_zeros_accumulate_switch_and_reset():
    """Noise-free sensor (E is derr) => noise exactly zero; no policy => zeta exactly zero; nfiltered = 0 => H_com
    exactly zero.  Frames stepped without `accumulate` do not count; reset() returns to frame 0."""
    import torch
    from ao_marl_amd import roket
    c = _case()
    na = c["na"]
    bank = roket.RoketBank(2, c["RD"], c["P"], c["Btt"], c["g"], c["gamma"], 0, 2)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v[:, :2])).to("cuda:0") for k, v in c["in"].items()}

    def run(first_accumulated):
        out = []
        for t in range(8):
            bank.step(dev["derr"][t], dev["derr"][t], dev["F"][t], dev["ageom"][t], dev["B"][t], None, None,
                      accumulate=t >= first_accumulated)
            x, b = bank.history()
            out.append(x.cpu().numpy())
            assert (x[0] == 0).all() and (b[0] == 0).all()          # noise, noise_buf
            assert (x[3] == 0).all()                                # H_com
            assert (x[5] == 0).all() and (b[2] == 0).all()          # tomography, tomo_buf
            assert (x[6] == 0).all()                                # zeta
            assert float(x[1].abs().max()) > 0 or t < 2             # the others are not: trunc from frame `delay` on
            assert float(x[4].abs().max()) > 0                      # bandwidth from frame 0 on
        return np.stack(out), bank.moments()

    xa, (S1, S2, n) = run(3)
    assert n == 5
    assert (S1[:, [0, 3, 5, 6]] == 0).all() and np.abs(S1[:, 4]).max() > 0
    bank.reset()
    assert bank.moments()[2] == 0 and (bank.moments()[1] == 0).all()
    xb, (T1, T2, m) = run(0)
    assert m == 8 and np.array_equal(xa, xb)
    with pytest.raises(ValueError, match="derr"):
        bank.step(dev["derr"][0][:, :na - 1], dev["E"][0], dev["F"][0], dev["ageom"][0], dev["B"][0])


# ------------------------------------------------------------------------------------- VecRoket: CPU side
def test_npz_keys_and_shapes():
    """C3: the reference's key names (save_in_hdf5) and [env][nactu][frames behind the preloop] histories."""
    from ao_marl_amd import roket
    _, s, cal = helpers.calibrated(NAME)
    na, nm, nsl, nf, pre, kept = s.nactu, cal.P.shape[0], s.nslope, 9, 4, 3
    rng = np.random.default_rng(1)
    hist = {"x": [rng.normal(size=(7, kept, na)) for _ in range(nf)]}
    for k, w in (("com", na), ("wf_com", na), ("slopes", nsl), ("alias_meas", nsl), ("trunc_meas", nsl)):
        hist[k] = [rng.normal(size=(kept, w)) for _ in range(nf)]
    res = dict(fitting=np.arange(5.), SR=np.arange(5.), SR2=None, cov=np.zeros((5, 6, 6)), cor=np.zeros((5, 6, 6)),
               centroid_gain=np.ones(5), centroid_gain2=np.ones(5))
    d = roket.npz_dict(hist, [2, 0], [4, 1], pre, res, cal, s.cmat)
    want = {"noise", "aliasing", "tomography", "filtered modes", "non linearity", "bandwidth", "wf_com", "zeta_com", "P",
            "Btt", "IF.data", "IF.indices", "IF.indptr", "TT", "fitting", "SR", "SR2", "cov", "cor", "centroid_gain",
            "centroid_gain2", "R", "D", "com", "slopes", "alias_meas", "trunc_meas"}
    assert want <= set(d) and "psfortho" not in d
    for k in ("noise", "aliasing", "tomography", "filtered modes", "non linearity", "bandwidth", "wf_com", "zeta_com", "com"):
        assert d[k].shape == (2, na, nf - pre), k
    for k in ("slopes", "alias_meas", "trunc_meas"):
        assert d[k].shape == (2, nsl, nf - pre), k
    assert np.array_equal(d["bandwidth"][0], np.stack(hist["x"])[pre:, 4, 2].T)
    assert d["P"].shape == (nm, na) and d["Btt"].shape == (na, nm) and d["R"].shape == (na, nsl) and d["D"].shape == (nsl, na)
    assert d["cov"].shape == (2, 6, 6) and list(d["fitting"]) == [4.0, 1.0] and np.isnan(d["SR2"])
    assert d["TT"].shape[1] == 2 and d["IF.indptr"].size == na - 2 + 1
    import io
    buf = io.BytesIO()
    np.savez(buf, **d)
    buf.seek(0)
    assert set(np.load(buf).files) == set(d)


def _fake_env(**kw):
    """The attributes _roket_supervisor reads, in a configuration it accepts; kw: dotted overrides."""
    from types import SimpleNamespace as NS
    from ao_marl_amd import params
    sim = NS(_twin=None, prefetch=False, pending_atmos=False)
    sup = NS(sim=sim, prefetch_atmos=False, reset_prefetch=None, gain=0.7, _env_gains=False, geo=object(),
             pure_delay_0=False, autoencoder=None, config=params.builtin(NAME))
    env = NS(supervisor=sup, frame_pipeline=False, rl_step=lambda *a, **k: None)
    for k, v in kw.items():
        obj, path = env, k.split("__")
        for p in path[:-1]:
            obj = getattr(obj, p)
        setattr(obj, path[-1], v)
    return env


def test_refusals_name_their_argument():
    """C4"""
    from ao_marl_amd import roket
    assert roket._roket_supervisor(_fake_env()) is not None
    for kw, exc, word in (
            (dict(frame_pipeline=True), RuntimeError, "frame_pipeline"),
            (dict(frame_pipeline="auto"), RuntimeError, "frame_pipeline"),
            (dict(supervisor__sim___twin=object()), RuntimeError, "frame_pipeline"),
            (dict(supervisor__prefetch_atmos=True), RuntimeError, "prefetch_atmos"),
            (dict(supervisor__sim__pending_atmos=True), RuntimeError, "prefetch_atmos"),
            (dict(supervisor__reset_prefetch="same"), RuntimeError, "reset_prefetch"),
            (dict(supervisor__gain=None), RuntimeError, "set_env_gains"),
            (dict(supervisor___env_gains=True), RuntimeError, "set_env_gains"),
            (dict(supervisor__geo=None), RuntimeError, "geo=True"),
            (dict(supervisor__pure_delay_0=True), NotImplementedError, "modification_online"),
            (dict(supervisor__autoencoder=object()), NotImplementedError, "autoencoder")):
        with pytest.raises(exc, match=word):
            roket._roket_supervisor(_fake_env(**kw))
    for mutate, word in ((lambda c: setattr(c.p_wfss[0], "xpos", 5.0), r"p_wfss\[0\]"),
                         (lambda c: setattr(c.p_targets[0], "ypos", -3.0), r"p_targets\[0\]"),
                         (lambda c: setattr(c.p_centroiders[0], "type", "tcog"), r"p_centroiders\[0\].type"),
                         (lambda c: setattr(c.p_centroiders[0], "type", "bpcog"), r"p_centroiders\[0\].type"),
                         (lambda c: setattr(c.p_wfss[0], "type", "pyrhr"), r"p_wfss\[0\].type")):
        env = _fake_env()
        mutate(env.supervisor.config)
        with pytest.raises(NotImplementedError, match=word):
            roket._roket_supervisor(env)
    with pytest.raises(TypeError):
        roket._roket_supervisor(object())


# ------------------------------------------------------------------------------------- VecRoket: GPU side
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)


def _noisy_params():
    from ao_marl_amd import params
    ps = params.builtin(NAME)
    ps.p_wfss[0].noise = 3.0
    return ps


def _snapshot(env):
    sup = env.supervisor
    return [t.clone() for t in (sup.sim.t["slopes"], sup.sim.t["com"], sup.sim.t["voltage"], sup.sim.t["strehl"],
                                sup.sim.t["frame"], sup.geo.t["com"], sup.geo.t["strehl"])]


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
def test_breakdown_leaves_the_loop_untouched_and_its_structural_zeros(noisy, tmp_path):
    """G3: the same 25 integrator frames with and without do_error_breakdown: slopes, commands, voltages, Strehl
    records (and the noise generator's frame counter, and the twin) bit for bit.  G4: noise-free sensor => noise and
    noise_buf exactly zero; no policy => zeta; coincident directions => tomography and tomo_buf."""
    import torch
    from ao_marl_amd.env import VecAoEnv
    from ao_marl_amd import roket
    cfg = _noisy_params() if noisy else NAME
    a = VecAoEnv(cfg, 4, RL, n_agents_modal=1, geo=True, frame_pipeline=False)
    b = VecAoEnv(_noisy_params() if noisy else NAME, 4, RL, n_agents_modal=1, geo=True, frame_pipeline=False)
    rk = roket.VecRoket(b, 25, 5, keep_envs=(0, 2), psf_ortho_envs=(1,))      # histories and full frames cost the loop nothing either
    sa, sb = a.reset(), b.reset()
    assert torch.equal(sa, sb)
    zero = torch.zeros(4, a.action_dim, device="cuda:0")
    for it in range(25):
        a.rl_step(zero, linear_control=True)
        b.rl_step(zero, linear_control=True, apply_control=False, compute_tar_psf=False)
        rk.do_error_breakdown()
        for u, v in zip(_snapshot(a), _snapshot(b)):
            assert torch.equal(u, v), it
        x, bufs = rk.bank.history()
        assert (x[6] == 0).all() and (x[5] == 0).all() and (bufs[2] == 0).all()
        if noisy:
            assert it < 2 or float(x[0].abs().max()) > 0
            assert float(bufs[0].abs().max()) > 0
        else:
            assert (x[0] == 0).all() and (bufs[0] == 0).all()
        assert float(x[4].abs().max()) > 0 and (it < 2 or float(x[2].abs().max()) > 0)
        sa, sb = a.linear_step(), b.linear_step()
        assert torch.equal(sa, sb), it
        for u, v in zip(_snapshot(a), _snapshot(b)):
            assert torch.equal(u, v), it
    res = rk.results()
    assert res["frames"] == 25 and res["cov"].shape == (4, 6, 6) and res["cor"].shape == (4, 6, 6)
    assert (res["cov"][:, 5] == 0).all() and (res["fitting"] > 0).all()
    assert res["var_modes"].shape == (4, 6, rk.nmodes) and res["var_agents"].shape[2] == len(res["agent_ranges"])
    assert np.allclose(res["var_modes"].sum(axis=2), np.diagonal(res["cov"], axis1=1, axis2=2))
    assert np.allclose(res["var_modes_sum"].sum(axis=1), res["cov"].sum(axis=(1, 2)))
    if not noisy:
        assert (res["cov"][:, 0] == 0).all()
        assert np.allclose(res["centroid_gain"], res["centroid_gain2"])
    # the .npz of the kept environments: 20 frames behind the preloop
    keys = rk.save(str(tmp_path / "budget.npz"), envs=[2])
    d = np.load(str(tmp_path / "budget.npz"))
    assert set(keys) == set(d.files) and d["bandwidth"].shape == (1, rk.nactu, 20) and d["slopes"].shape == (1, rk.nslope, 20)
    assert d["psfortho"].shape == (1, b.supervisor.s.npsf, b.supervisor.s.npsf) and float(d["psfortho"].max()) > 0
    assert (d["tomography"] == 0).all() and np.array_equal(d["cov"][0], res["cov"][2])
    with pytest.raises(ValueError, match="keep_envs"):
        rk.save(str(tmp_path / "x.npz"), envs=[1])


@pytest.mark.gpu
def test_breakdown_against_the_oracle():
    """G5: 2 environments, 12 integrator frames, the HIP screens copied to the oracle every frame.  derr, E, F,
    ageom, B and the seven contributors per frame within 2e-3 of max|com| of controller 0 (the project's command
    tolerance, tests/test_geo.py)."""
    import torch
    from oracle import aoref
    from ao_marl_amd.env import VecAoEnv
    from ao_marl_amd import roket
    env = VecAoEnv(NAME, 2, RL, n_agents_modal=1, geo=True, frame_pipeline=False)
    sup = env.supervisor
    sim, s, cal = sup.sim, sup.s, sup.cal
    rk = roket.VecRoket(env, 12, 0)
    env.reset()
    na = s.nactu
    oracles = [aoref.OracleSim(s, seed=int(sd)) for sd in sup.env_seeds()]
    geos = [aoref.OracleGeo(o, cal.IF) for o in oracles]
    oroks = [rr.OracleRoket(o, g, cal.IF, rk.RD, cal.P, cal.Btt, rk.nfiltered) for o, g in zip(oracles, geos)]

    def oracle_frame():
        for l in range(s.nscreens):
            scr = sim.screen(l).cpu().numpy()
            for e, o in enumerate(oracles):
                o.screens[l] = scr[e].copy()
        for o, g in zip(oracles, geos):                    # next_part_one without move_atmos: the screens are the HIP side's
            o.raytrace_target()
            o.raytrace_wfs(atm=True, dms=False, reset=True)
            o.raytrace_wfs(atm=False, dms=True, reset=False)
            o.comp_image()
            o.do_centroids()
            o.do_control()
            g.next_part_one_geo()

    oracle_frame()
    zero = torch.zeros(2, env.action_dim, device="cuda:0")
    hip = {k: [] for k in ("derr", "E", "F", "ageom", "B", "x", "fit")}
    scale = 0.0
    for it in range(12):
        env.rl_step(zero, linear_control=True, apply_control=False, compute_tar_psf=False)
        rk.do_error_breakdown()
        for k, t in (("derr", rk.derr), ("E", rk.derr), ("F", rk.F), ("ageom", rk.ageom), ("B", sup.geo.t["com"])):
            hip[k].append(t[:, :na].cpu().numpy().copy())
        hip["x"].append(rk.bank.history()[0].cpu().numpy())
        hip["fit"].append(sup.geo.t["strehl"][:, 2].cpu().numpy().copy())
        for o, k in zip(oracles, oroks):
            k.breakdown()
            o.next_part_two(None)
            scale = max(scale, float(np.abs(o.com).max()))
        env.linear_step()
        oracle_frame()
    bound = 2e-3 * scale
    worst = {}
    for e, k in enumerate(oroks):
        want = k.contributors()
        for name in ("derr", "E", "F", "ageom", "B"):
            d = np.abs(np.stack(hip[name])[:, e] - np.stack(k.rec[name])).max()
            worst[name] = max(worst.get(name, 0.0), float(d))
        for i, name in enumerate(rr.NAMES):
            d = np.abs(np.stack(hip["x"])[:, i, e] - want[name]).max()
            worst[name] = max(worst.get(name, 0.0), float(d))
            print("env %d %-6s max|x| = %.4g" % (e, name, np.abs(want[name]).max()))
        fit = np.abs(np.stack(hip["fit"])[:, e] - np.stack(k.rec["fit"])).max() / np.stack(k.rec["fit"]).max()
        worst["fit(rel)"] = max(worst.get("fit(rel)", 0.0), float(fit))
    for name, d in worst.items():
        print("G5 %-8s |hip - oracle| = %.3e = %.3e of max|com| (%.4g); bound %.3e" % (name, d, d / scale, scale, bound))
    for name, d in worst.items():
        if name != "fit(rel)":
            assert d < bound, (name, d, bound)
    assert worst["fit(rel)"] < 2e-2                         # the twin's phase variance, as tests/test_geo.py bounds it


def _zeta_check(rl_hist, x_hist, rk, cal):
    """zeta of the run against filter_bank_f64 fed with the rl_com read back, under G1's bound"""
    nf, nenv, na = rl_hist.shape
    z = np.zeros((nf, na))
    worst = 0.0
    for e in range(nenv):
        args = (z, z, z, z, z, None, rl_hist[:, e], rk.RD, cal.P, cal.Btt, rk.g, rk.gamma, rk.nfiltered, rk.delay)
        h64 = rr.filter_bank_f64(*args)["zeta"]
        h32 = rr.filter_bank_f64(*args, dtype=np.float32)["zeta"]
        ref_err = np.abs(h32 - h64).max()
        err = np.abs(x_hist[:, e] - h64).max()
        print("zeta env %d: |hip - f64| = %.3e, |np32 - f64| = %.3e, max = %.3g" % (e, err, ref_err, np.abs(h64).max()))
        assert err <= 8 * ref_err + 1e-6 * np.abs(rl_hist).max(), (e, err, ref_err)
        worst = max(worst, float(np.abs(h64).max()))
    return worst


@pytest.mark.gpu
def test_breakdown_with_a_policy():
    """G6: a policy with a small non-zero mean head, 4 environments, 20 frames: zeta is the bank's recursion on
    Btt . (rl * freedom) as read back from the run, and the tables are 7x7."""
    import torch
    from ao_marl_amd.env import VecAoEnv
    from ao_marl_amd.agents import BatchedGaussianPolicy
    from ao_marl_amd import roket
    env = VecAoEnv(NAME, 4, RL, n_agents_modal=1, geo=True, frame_pipeline=False)
    pol = BatchedGaussianPolicy(env.layout)
    g = torch.Generator(device="cpu").manual_seed(5)
    with torch.no_grad():
        pol.Wm.copy_((torch.rand(pol.Wm.shape, generator=g) * 2 - 1).to(pol.Wm.device) * 1e-3)
        pol.bm.copy_((torch.rand(pol.bm.shape, generator=g) * 2 - 1).to(pol.bm.device) * 0.05)
    pol._native, pol._desc = None, None
    rk = roket.VecRoket(env, 20, 0, policy=pol)
    s = env.reset()
    rl_hist, x_hist = [], []
    for it in range(20):
        a = pol.select_action(s, eval_mode=True)[0]
        env.rl_step(a, apply_control=False, compute_tar_psf=False)
        rk.do_error_breakdown(a)
        rl_hist.append(rk.rl_com[:, :rk.nactu].cpu().numpy().copy())
        x_hist.append(rk.bank.history()[0][6].cpu().numpy())
        # rl_com is Btt . (action * freedom) on the action range
        fv = np.asarray(env.supervisor.freedom_vector, dtype=np.float64)
        ar = np.asarray(env.supervisor.obtain_action_range_modal()) % rk.nmodes
        m = np.zeros((4, rk.nmodes))
        m[:, ar] = a.double().cpu().numpy() * fv[ar]
        want = m @ np.asarray(env.supervisor.cal.Btt, dtype=np.float64).T
        assert np.abs(rl_hist[-1] - want).max() < 1e-5 * np.abs(want).max() + 1e-12
        s = env.linear_step()
    rl_hist, x_hist = np.stack(rl_hist), np.stack(x_hist)
    assert np.abs(rl_hist).max() > 0
    assert _zeta_check(rl_hist, x_hist, rk, env.supervisor.cal) > 0
    res = rk.results()
    assert res["cov"].shape == (4, 7, 7) and (res["cov"][:, 6, 6] > 0).all() and len(res["contributors"]) == 7
    assert np.allclose(np.diagonal(res["cor"], axis1=1, axis2=2)[:, [1, 2, 3, 4, 6]], 1.0)


@pytest.mark.gpu
def test_breakdown_on_a_noisy_sensor():
    """G7: the noise contributor is non-zero and is the bank's recursion on derr - E, with E from a noise-free second
    formation of the same phase that the test does itself on the loop's own state (and puts back)."""
    import torch
    from ao_marl_amd.env import VecAoEnv
    from ao_marl_amd import roket
    env = VecAoEnv(_noisy_params(), 2, RL, n_agents_modal=1, geo=True, frame_pipeline=False)
    sup = env.supervisor
    sim, s, cal = sup.sim, sup.s, sup.cal
    rk = roket.VecRoket(env, 16, 0)
    assert rk.noisy
    env.reset()
    zero = torch.zeros(2, env.action_dim, device="cuda:0")
    noisy_sl, clean_sl, x_hist = [], [], []
    for it in range(16):
        env.rl_step(zero, linear_control=True, apply_control=False, compute_tar_psf=False)
        keep, frame = sim.t["slopes"].clone(), sim.t["frame"].clone()
        sim.comp_image(noise=False, cog=True)
        clean_sl.append(sim.t["slopes"].cpu().numpy().copy())
        sim.t["slopes"].copy_(keep)
        sim.t["frame"].copy_(frame)
        noisy_sl.append(keep.cpu().numpy())
        rk.do_error_breakdown()
        x_hist.append(rk.bank.history()[0][0].cpu().numpy())
        env.linear_step()
    noisy_sl, clean_sl, x_hist = np.stack(noisy_sl), np.stack(clean_sl), np.stack(x_hist)
    assert np.abs(x_hist).max() > 0 and np.abs(noisy_sl - clean_sl).max() > 0
    z = np.zeros((16, s.nactu))
    for e in range(2):
        out = {}
        for dt in (np.float64, np.float32):
            cm = np.asarray(s.cmat, dtype=dt)
            derr, E = -(noisy_sl[:, e].astype(dt) @ cm.T), -(clean_sl[:, e].astype(dt) @ cm.T)
            out[dt] = rr.filter_bank_f64(derr, E, z, z, z, None, None, rk.RD, cal.P, cal.Btt, rk.g, rk.gamma,
                                         rk.nfiltered, rk.delay, dtype=dt)["noise"]
            scale = float(np.abs(derr).max())
        ref_err = np.abs(out[np.float32] - out[np.float64]).max()
        err = np.abs(x_hist[:, e] - out[np.float64]).max()
        print("noise env %d: |hip - f64| = %.3e, |np32 - f64| = %.3e, max|noise| = %.3g, max|derr| = %.3g" %
              (e, err, ref_err, np.abs(out[np.float64]).max(), scale))
        assert err <= 8 * ref_err + 1e-6 * scale, (e, err, ref_err)
