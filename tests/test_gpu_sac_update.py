"""aomarl_sac_update (csrc/aomarl_sac.hip) against the float64 statement of the update (tests/sac_reference.py, pinned
to the reference's own update by tests/test_sac_reference.py), stage by stage, on the cases of tests/sac_cases.py.

Bounds: per tensor max|g - g64| / max|g64| and the relative error of each loss <= 4 x the floors
recorded in tests/sac_cases.py = 4 x what torch's own float32 autograd on the CPU deviates from float64 by on these
inputs; Adam, the soft update and the temperature to 2 ulp of float32 of float64 arithmetic on the kernel's own
gradients and moments (parameters of the step's own size: _adam_distance); padding, clamped and saturated columns
exactly zero.  Every test prints what it measured."""
import numpy as np
import pytest
import torch

from tests import sac_cases as cases
from tests import sac_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND_CRITIC, BOUND_POLICY = cases.FACTOR * cases.FLOOR_CRITIC, cases.FACTOR * cases.FLOOR_POLICY


def _device_sac(name, monkeypatch):
    """A native BatchedSAC on the GPU holding the case's parameters and replay rows."""
    c = cases.case(name)
    if name == "aligned_gen":
        monkeypatch.setenv("AOMARL_SAC_GEMM", "gen")           # read when the updater is created
    else:
        monkeypatch.delenv("AOMARL_SAC_GEMM", raising=False)
    sac = cases.new_sac(name, device=DEV, native=True)
    with torch.no_grad():
        for dst, src in ((sac._pflat, c.sac._pflat), (sac._cflat, c.sac._cflat), (sac._ctflat, c.sac._ctflat),
                         (sac.log_alpha, c.sac.log_alpha), (sac.alpha, c.sac.alpha)):
            dst.copy_(src.detach())
    d = c.data
    sac.memory.push(d["state"].to(DEV), d["action"].to(DEV), d["reward"].to(DEV), d["next_state"].to(DEV),
                    d["mask"].to(DEV))
    assert len(sac.memory) == c.rows
    if c.edge == "short_ring":                                 # whatever lies past the filled part poisons the update
        m = sac.memory
        for buf in (m.state, m.next_state, m.action, m.reward, m.mask):
            buf[c.rows:] = float("nan")
    sac.updater(c.B)
    return c, sac


def _update(sac, c, u, own_draws=False):
    if own_draws:
        sac.update_from_memory(c.B)
    else:
        sac.update_from_memory(c.B, c.idx[u].to(DEV).contiguous(), c.eps_next[u].to(DEV).contiguous(),
                               c.eps_pi[u].to(DEV).contiguous())
    torch.cuda.synchronize()


def _state(sac, c):
    """Everything the update reads or writes, on the host."""
    u = sac.updater(c.B)
    h = lambda t: t.detach().cpu().clone()        # noqa: E731
    lo = sac.last_losses
    return dict(p=h(sac._pflat), c=h(sac._cflat), ct=h(sac._ctflat), la=h(sac.log_alpha).reshape(-1),
                alpha=h(sac.alpha), gp=h(u.policy_grad), gc=h(u.critic_grad), gla=h(u.la_grad),
                pm=h(u.policy_m), pv=h(u.policy_v), cm=h(u.critic_m), cv=h(u.critic_v), lam=h(u.la_m), lav=h(u.la_v),
                losses=None if lo is None else {k: h(v).reshape(-1) for k, v in lo.items()})


def _stage_errors(c, after, cref, aref, tuned):
    return cases.stage_errors(c, cases.split_critic(c, after["gc"]), cases.split_policy(c, after["gp"]),
                              after["gla"] if tuned else None, after["losses"], cref, aref)


def _assert_stages(label, ec, ep, extra_policy=0.0):
    print("%s: critic worst %.2e of %.1e (%s); policy side worst %.2e of %.1e (%s)" %
          (label, max(ec.values()), BOUND_CRITIC, cases.fmt(ec), max(ep.values()), BOUND_POLICY + extra_policy,
           cases.fmt(ep)))
    assert max(ec.values()) <= BOUND_CRITIC, (label, ec)
    assert max(ep.values()) <= BOUND_POLICY + extra_policy, (label, ep)


def _ulp_distance(got, want):
    """|got - want| in units of float32's spacing at want (want: float64)"""
    want = want.detach().double().numpy()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return np.abs(got.detach().double().numpy() - want) / ulp


def _adam_distance(got, want, before, lr):
    """(worst ulp distance over the parameters of ordinary size, worst error / allowance over the small ones, their number)

    2 ulp of float32 at the expected value holds where Adam's step is small beside the parameter: the step's own
    rounding is then far below the parameter's spacing.  A parameter of the step's own size is another matter: at
    p = -3.010e-4 and a step of 3.000e-4 the result is -1.0e-6, and the step's float32 rounding (3e-11) is 150 ulp of
    THAT (float32 Adam restated in NumPy on the `aligned` case: 149 ulp there, 0.7 ulp over the entries with
    |p| >= 8 lr).  So: |p| >= 8 lr (the step, about lr, rounds to 5 ulp of itself at worst: below 0.7 ulp of p):
    2 ulp at the expected value; smaller |p|: 2 ulp at the expected value + 4 ulp at the larger of the step and lr (the
    step passes through about ten float32 roundings, those of v halved by the root: 5 ulp at worst, 1.9 measured in the
    restatement; from the second update on m + (g - m) / 10 can cancel, and the step, lr times a ratio of order one,
    then rounds at the size of that ratio's terms: lr, not the step)."""
    before, want64 = before.detach().double().numpy(), want.detach().double().numpy()
    err = np.abs(got.detach().double().numpy() - want64)
    sp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)      # noqa: E731
    big = np.abs(before) >= 8.0 * lr
    small_err = err[~big] / (2.0 * sp(want64[~big]) + 4.0 * sp(np.maximum(np.abs(want64[~big] - before[~big]), lr)))
    return float((err[big] / sp(want64[big])).max()), float(small_err.max()) if small_err.size else 0.0, int((~big).sum())


# ------------------------------------------------------------------------------------------ U1
@pytest.mark.parametrize("name", cases.TABLE + cases.EDGE)
def test_u1_gradients_and_losses_of_the_first_update_match_float64(name, monkeypatch):
    """Critic gradients and q losses against critic_stage on the case's parameters; policy gradients, policy loss and
    the temperature gradient against actor_stage on the critic read back from the device, temperature from before."""
    c, sac = _device_sac(name, monkeypatch)
    _update(sac, c, 0)
    after = _state(sac, c)
    ec, ep = _stage_errors(c, after, cases.critic_reference(name), cases.actor_reference(name, after["c"]),
                           sac.automatic_entropy_tuning)
    _assert_stages("U1 %s" % name, ec, ep)


# ------------------------------------------------------------------------------------------ U2
def _padding(c):
    """[(tensor label, index of flat-buffer view, agent, slices of the padded part)] for policy and critic"""
    L = c.L
    names = cases.POLICY_NAMES(L)
    pol, cri = [], []
    for i, (ni, na) in enumerate(zip(c.sac.ins, c.sac.acts)):
        if ni < c.I:
            pol.append((names.index("W1"), (i, slice(ni, None))))
            cri.append(("Win", (i, slice(ni, c.I))))
        if na < c.Na:
            for n in ("Wm", "Ws", "bm", "bs"):
                pol.append((names.index(n), (i, slice(None), slice(na, None))))
            cri.append(("Win", (i, slice(c.I + na, None))))
    return pol, cri


@pytest.mark.parametrize("name", cases.TABLE)
def test_u2_padding_has_zero_gradient_and_never_moves(name, monkeypatch):
    c, sac = _device_sac(name, monkeypatch)
    pol, cri = _padding(c)
    assert pol and cri
    before = _state(sac, c)
    for u in range(cases.N_UPDATES):
        _update(sac, c, u)
        s = _state(sac, c)
        gp, gc = cases.split_policy(c, s["gp"]), cases.split_critic(c, s["gc"])
        p, q = cases.split_policy(c, s["p"]), cases.split_critic(c, s["c"])
        p0, q0 = cases.split_policy(c, before["p"]), cases.split_critic(c, before["c"])
        for j, where in pol:
            assert gp[j][where].numel() > 0
            assert float(gp[j][where].abs().max()) == 0.0, (u, j, where)
            assert torch.equal(p[j][where], p0[j][where]) and float(p[j][where].abs().max()) == 0.0, (u, j, where)
        for k, where in cri:
            for t in range(2):
                assert gc[t][k][where].numel() > 0
                assert float(gc[t][k][where].abs().max()) == 0.0, (u, t, where)
                assert torch.equal(q[t][k][where], q0[t][k][where]), (u, t, where)
    assert not torch.equal(s["p"], before["p"]) and not torch.equal(s["c"], before["c"])


def test_u2_clamped_columns_have_exactly_zero_log_std_gradient(monkeypatch):
    c, sac = _device_sac("clamped", monkeypatch)
    _update(sac, c, 0)
    gp = cases.split_policy(c, _state(sac, c)["gp"])
    Ws, bs, Wm = gp[-2], gp[-1], gp[-4]
    for i, na in enumerate(c.sac.acts):
        hi, lo, mid = cases.clamped_columns(na)
        for cols in (hi, lo):                                  # both sides of the clamp gate: dls = 0
            assert float(Ws[i][:, cols].abs().max()) == 0.0 and float(bs[i][:, cols].abs().max()) == 0.0
            assert float(Wm[i][:, cols].abs().max()) > 0.0     # (the mean of those columns still learns)
        if len(mid):
            assert float(Ws[i][:, mid].abs().max()) > 0.0 and float(bs[i][:, mid].abs().min()) > 0.0


def test_u2_saturated_columns_have_zero_mean_gradient_and_the_capped_log_probability(monkeypatch):
    """tanhf is exactly +-1 there: d tanh = 0, so bm's gradient is exactly 0, and the tanh correction of such a column
    is -log(1e-5) exactly."""
    c, sac = _device_sac("saturated", monkeypatch)
    _update(sac, c, 0)
    s = _state(sac, c)
    bm = cases.split_policy(c, s["gp"])[-3]
    aref = cases.actor_reference("saturated", s["c"])
    eps = c.eps_pi[0].double()
    log_std = aref["raw"].clamp(R.LOG_SIG_MIN, c.log_sig_max)
    normal = -0.5 * eps * eps - log_std - 0.5 * np.log(2 * np.pi)
    corr = -torch.log(1.0 - torch.tanh(aref["pre_tanh"]) ** 2 + R.EPSILON)
    for i, na in enumerate(c.sac.acts):
        sat = torch.cat(cases.saturated_columns(na))
        assert float(bm[i][:, sat].abs().max()) == 0.0
        rest = torch.ones(na, dtype=torch.bool)
        rest[sat] = False
        assert float(bm[i, 0, :na][rest].abs().min()) > 0.0
        corr[i][:, sat] = -np.log(1e-5)
    want = ((normal + corr) * c.act_mask.double()).sum(dim=2).mean(dim=1)          # mean log pi per agent
    got = -s["gla"].double() - c.target_entropy.reshape(-1).double()               # la_grad = -(mean log pi + te)
    err = float(((got - want).abs() / want.abs()).max())
    print("U2 saturated: mean log pi %s, with -log(1e-5) per saturated column %s, relative error %.2e of %.1e" %
          (got.tolist(), want.tolist(), err, BOUND_POLICY))
    assert err <= BOUND_POLICY


def test_u2_short_ring_never_reads_past_the_filled_rows(monkeypatch):
    """Own draws on a ring of 64 with 7 rows pushed and NaN everywhere behind them: one NaN shows a row drawn past
    len(memory)."""
    c, sac = _device_sac("short_ring", monkeypatch)
    for u in range(cases.N_UPDATES):
        _update(sac, c, u, own_draws=True)
        s = _state(sac, c)
        for k in ("gp", "gc", "gla", "p", "c", "ct"):
            assert bool(torch.isfinite(s[k]).all()), (u, k)
        assert all(bool(torch.isfinite(v).all()) for v in s["losses"].values()), u
        assert float(s["gp"].abs().max()) > 0 and float(s["gc"].abs().max()) > 0


# ------------------------------------------------------------------------------------------ U3
@pytest.mark.parametrize("name", ["aligned", "odd_hidden", "fixed_alpha"])
def test_u3_adam_soft_update_and_temperature_follow_the_kernels_own_gradients(name, monkeypatch):
    """Updates 1-3, each judged on what the kernel itself had: its gradients, its moments and its parameters from before
    the update.  The target critic is bit-equal on steps without a soft update; a fixed temperature never moves."""
    c, sac = _device_sac(name, monkeypatch)
    f32 = lambda v: float(np.float32(v))        # noqa: E731  (what the library's descriptor holds)
    hyper = dict(lr=f32(sac.lr), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))
    tau, omt = f32(sac.tau), float(np.float32(1.0) - np.float32(sac.tau))
    tuned = sac.automatic_entropy_tuning
    for t in range(1, cases.N_UPDATES + 1):
        s0 = _state(sac, c)
        _update(sac, c, t - 1)
        s1 = _state(sac, c)
        worst, small = {}, {}
        for key, g, m, v in (("p", "gp", "pm", "pv"), ("c", "gc", "cm", "cv")):
            want, wm, wv = R.adam(s0[key], s1[g], s0[m], s0[v], t, **hyper)
            worst[key], small[key], nsmall = _adam_distance(s1[key], want, s0[key], hyper["lr"])
            assert nsmall < 0.6 * want.numel()
            assert float((s1[key] - s0[key]).abs().max()) > 0, (t, key)            # it moved
            # the moments it leaves behind (the next step starts from them): 2 ulp at the size of their terms
            gg = s1[g].double()
            for got, ref, scale in ((s1[m], wm, torch.maximum(s0[m].double().abs(), gg.abs())),
                                    (s1[v], wv, torch.maximum(s0[v].double(), gg * gg))):
                ulp = np.spacing(scale.clamp(min=1e-30).numpy().astype(np.float32)).astype(np.float64)
                assert float((np.abs(got.double().numpy() - ref.numpy()) / ulp).max()) <= 2.0, (t, key)
        if t % sac.target_update_interval == 0:
            # (1 - tau) old + tau new, judged at the larger of the old value and the result: each term rounds at its own
            # size, and where the two nearly cancel (a critic weight that changed sign) the result is far smaller than both
            want = R.soft_update(s0["ct"], s1["c"], tau, omt)
            at = torch.where(want.abs() >= s0["ct"].double().abs(), want, s0["ct"].double())
            worst["ct"] = float((np.abs(s1["ct"].double().numpy() - want.numpy()) /
                                 np.spacing(np.abs(at.numpy()).astype(np.float32)).astype(np.float64)).max())
            assert float((s1["ct"] - s0["ct"]).abs().max()) > 0, t
        else:
            assert torch.equal(s1["ct"], s0["ct"]), t
        if tuned:
            want, _, _ = R.adam(s0["la"], s1["gla"], s0["lam"], s0["lav"], t, **hyper)
            worst["log_alpha"] = float(_ulp_distance(s1["la"], want).max())
            worst["alpha"] = float(_ulp_distance(s1["alpha"].reshape(-1), s1["la"].double().exp()).max())
            assert float((s1["la"] - s0["la"]).abs().max()) > 0, t
        else:
            assert torch.equal(s1["la"], s0["la"]) and torch.equal(s1["alpha"], s0["alpha"]), t
            assert torch.equal(s1["la"], c.sac.log_alpha.detach().reshape(-1)) and torch.equal(s1["alpha"], c.alpha)
            assert float(s1["losses"]["alpha"].abs().max()) == 0.0
        assert torch.equal(s1["losses"]["alpha_value"], s1["alpha"].reshape(-1))
        print("U3 %s step %d: worst ulp distance %s; parameters below 8 lr, error / allowance: %s" %
              (name, t, " ".join("%s %.2f" % kv for kv in worst.items()), " ".join("%s %.2f" % kv for kv in small.items())))
        assert max(worst.values()) <= 2.0, (t, worst)
        assert max(small.values()) <= 1.0, (t, small)


# ------------------------------------------------------------------------------------------ U4
@pytest.mark.parametrize("name", ["aligned", "odd_head"])
def test_u4_own_draws_are_the_documented_philox_streams(name, monkeypatch):
    """Without rows and normals the kernels draw them from Philox: rows from stream 11, eps_next from stream 12 and
    eps_pi from stream 13, in the sample AND in its backward pass.  Updates 1 and 3 against the float64 stages
    evaluated at the restated draws: a wrong row is a gross error everywhere, a backward pass that recomputes another
    normal than the forward pass a gross error in the policy gradient alone."""
    c, sac = _device_sac(name, monkeypatch)
    tuned = sac.automatic_entropy_tuning
    for step in range(1, cases.N_UPDATES + 1):
        s0 = _state(sac, c)
        assert sac.total_update + 1 == step
        _update(sac, c, step - 1, own_draws=True)
        if step == 2:
            continue
        s1 = _state(sac, c)
        idx, e_next, e_pi = R.draws(sac.seed, step, c.A, c.B, c.Na, c.rows)
        batch = cases.gather_batch(c, idx)
        pol = R.policy_dict(cases.split_policy(c, s0["p"]))
        cref = cases.critic_reference_at(c, pol, cases.split_critic(c, s0["c"]), cases.split_critic(c, s0["ct"]),
                                         s0["alpha"], batch, e_next)
        aref = cases.actor_reference_at(c, pol, cases.split_critic(c, s1["c"]), s0["alpha"], batch, e_pi)
        ec, ep = _stage_errors(c, s1, cref, aref, tuned)
        _assert_stages("U4 %s update %d" % (name, step), ec, ep)


# ------------------------------------------------------------------------------------------ U5
def test_u5_the_env_switch_selects_the_other_product_path(monkeypatch):
    """aligned and aligned_gen both pass U1; they are different kernels all the same: summation order differs, so the
    critics' Win gradients are not bit-identical (and agree to twice the U1 bound)."""
    g = {}
    for name in ("aligned", "aligned_gen"):
        c, sac = _device_sac(name, monkeypatch)
        _update(sac, c, 0)
        g[name] = cases.split_critic(c, _state(sac, c)["gc"])
    for t in range(2):
        a, b = g["aligned"][t]["Win"], g["aligned_gen"][t]["Win"]
        assert not torch.equal(a, b)
        assert cases.tensor_error(a, b) <= 2 * BOUND_CRITIC
