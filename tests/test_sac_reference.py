"""The float64 statement of the SAC update (tests/sac_reference.py) and the cases the GPU test runs it on
(tests/sac_cases.py), CPU side: the statement against the reference's own update (golden fixture), the condition on the
inputs that the GPU bounds rest on, the edge cases' branches, and the restated Philox draws."""
import os

import numpy as np
import pytest
import torch

from ao_marl_amd.agents import AgentLayout, LOG_SIG_MIN
from ao_marl_amd.sac import BatchedSAC
from tests import sac_cases as cases
from tests import sac_reference as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_sac_update.pt")


def _pad(t, width):
    out = t.new_zeros(t.shape[0], width)
    out[:, :t.shape[1]] = t
    return out


def _golden_run(dtype):
    """The stages chained over the fixture's three updates in `dtype` (Adam and the soft update as well):
    [update][agent] -> dict(losses, alpha, actor, critic, target) in the reference's checkpoint layout."""
    g = torch.load(GOLD)
    h = g["hyper"]
    lay = AgentLayout(87, [0, 80], 1, include_tip_tilt=True, n_filtered=5)
    # the package's object only carries the reference's checkpoints into the stacked layout and back out of it
    sac = BatchedSAC(lay, dict(hidden_size_actor=h["hidden"], hidden_size_critic=h["hidden"], memory_size=8,
                               initialize_last_layer_0=False), device="cpu")
    for i, ag in enumerate(g["agents"]):
        sac.load_reference_agent(i, ag["policy0"], ag["critic0"])
    A, out = sac.A, []
    with R.precision(dtype):
        pol = [t.detach().to(dtype).clone() for t in sac._policy_params()]
        cri = [{k: q[k].detach().to(dtype).clone() for k in R.CRITIC_KEYS} for q in sac.critic]
        tgt = [{k: q[k].detach().to(dtype).clone() for k in R.CRITIC_KEYS} for q in sac.critic_target]
        log_alpha, alpha = torch.zeros(A, dtype=dtype), torch.full((A, 1, 1), 0.2, dtype=dtype)
        te = sac.target_entropy
        pm, pv = [torch.zeros_like(t) for t in pol], [torch.zeros_like(t) for t in pol]
        cm = [{k: torch.zeros_like(q[k]) for k in q} for q in cri]
        cv = [{k: torch.zeros_like(q[k]) for k in q} for q in cri]
        lam, lav = torch.zeros(A, dtype=dtype), torch.zeros(A, dtype=dtype)
        for u in range(h["updates"]):
            ups = [ag["updates"][u] for ag in g["agents"]]
            batch = dict(x=torch.stack([_pad(t["s"], sac.in_max) for t in ups]),
                         x2=torch.stack([_pad(t["s2"], sac.in_max) for t in ups]),
                         a=torch.stack([_pad(t["a"], sac.act_max) for t in ups]),
                         r=torch.stack([t["r"] for t in ups]), mask=torch.stack([t["mask"] for t in ups]))
            e1 = torch.stack([_pad(t["eps_next"], sac.act_max) for t in ups])
            e2 = torch.stack([_pad(t["eps_pi"], sac.act_max) for t in ups])
            step = u + 1
            cs = R.critic_stage(R.policy_dict(pol), cri, tgt, alpha, batch, e1, h["gamma"], sac.act_mask, 2.0)
            for q in range(2):
                for k in R.CRITIC_KEYS:
                    cri[q][k], cm[q][k], cv[q][k] = R.adam(cri[q][k], cs["grads"][k][q], cm[q][k], cv[q][k], step, h["lr"])
            ac = R.actor_stage(R.policy_dict(pol), cri, alpha, batch, e2, sac.act_mask, 2.0)
            for j in range(len(pol)):
                pol[j], pm[j], pv[j] = R.adam(pol[j], ac["grads"][j], pm[j], pv[j], step, h["lr"])
            al_loss = R.alpha_loss(log_alpha, ac["mean_log_pi"], te)
            log_alpha, lam, lav = R.adam(log_alpha, R.alpha_grad(ac["mean_log_pi"], te), lam, lav, step, h["lr"])
            alpha = log_alpha.exp().reshape(A, 1, 1)
            for q in range(2):
                for k in R.CRITIC_KEYS:
                    tgt[q][k] = R.soft_update(tgt[q][k], cri[q][k], h["tau"])
            with torch.no_grad():
                for dst, src in zip(sac._policy_params(), pol):
                    dst.copy_(src)
                for qs, src in ((sac.critic, cri), (sac.critic_target, tgt)):
                    for q in range(2):
                        for k in R.CRITIC_KEYS:
                            qs[q][k].copy_(src[q][k])
            rec = []
            for i in range(A):
                snap = lambda sd: {k: v.clone() for k, v in sd.items()}      # noqa: E731  (some entries are views)
                actor, critic = (snap(sd) for sd in sac.export_agent(i))
                rec.append(dict(losses=dict(q1_loss=cs["q1_loss"][i].item(), q2_loss=cs["q2_loss"][i].item(),
                                            policy_loss=ac["policy_loss"][i].item(), alpha_loss=al_loss[i].item()),
                                alpha=alpha[i].item(), policy=actor, critic=critic,
                                critic_target=snap(sac.export_agent(i, target=True)[1])))
            out.append(rec)
    # padding never learns anything
    assert pol[0][1, 8:].abs().max().item() == 0.0 and pol[-4][1, :, 2:].abs().max().item() == 0.0
    assert cri[0]["Win"][1, 8:sac.in_max].abs().max().item() == 0.0
    return g, out


def test_statement_reproduces_the_references_sac_update():
    """tests/golden/host_sac_update.pt is the reference's own update_critic / update_actor / update_alpha /
    soft_update on its own modules in float32: two agents, three updates, recorded draws, an unscaled head.

    Evaluated in the fixture's own precision, the stages chained with their Adam and soft update give every loss, the
    temperature and every parameter of all three updates to the bounds
    test_sac.py::test_batched_update_reproduces_the_references_sac_update holds BatchedSAC.update to.

    In float64 the first update's losses agree to that bound plus what the statement itself changes by between float32
    and float64 (the fixture's round-off: 1 - y^2 cancels on its 80-column head; 1.2e-5 relative on that agent's policy
    loss).  Its parameters cannot be held to 2e-6 in float64, nor anything of updates 2 and 3: Adam's first step is
    lr g / (|g| + 1e-8), so entries whose float32 gradient is round-off move by up to 2 lr = 6e-4 (measured: 5.9e-4 on
    linear1.weight) -- the reason the stages are judged one by one everywhere else."""
    g, run32 = _golden_run(torch.float32)
    for u, (rec, ups) in enumerate(zip(run32, [[ag["updates"][u] for ag in g["agents"]] for u in range(3)])):
        for i, (got, t) in enumerate(zip(rec, ups)):
            for name, v in got["losses"].items():
                assert abs(v - t[name]) < 1e-5 * max(1, abs(t[name])), (u, i, name)
            assert abs(got["alpha"] - t["alpha"]) < 1e-6
            for part in ("policy", "critic", "critic_target"):
                for name, want in t[part].items():
                    assert torch.allclose(got[part][name], want, atol=2e-6, rtol=1e-5), (u, i, part, name)
    _, run64 = _golden_run(torch.float64)
    for i, t in enumerate(ag["updates"][0] for ag in g["agents"]):
        for name, v in run64[0][i]["losses"].items():
            own = abs(v - run32[0][i]["losses"][name])
            print("update 1, agent %d, %s: float64 %.9g, fixture %.9g, float32 statement off float64 by %.2e" %
                  (i, name, v, t[name], own))
            assert abs(v - t[name]) < 1e-5 * max(1, abs(t[name])) + own, (i, name)
        assert abs(run64[0][i]["alpha"] - t["alpha"]) < 1e-6


def _float32_deviation(name):
    c = cases.case(name)
    f32 = cases.float32_statement(name)
    cref = cases.critic_reference(name)
    aref = cases.actor_reference(name, f32["critic_after"])
    cg = [{k: f32["critic"][k][q] for k in R.CRITIC_KEYS} for q in range(2)]
    return cases.stage_errors(c, cg, f32["policy"], f32["la_grad"], f32["losses"], cref, aref)


@pytest.mark.parametrize("name", cases.TABLE + cases.EDGE)
def test_inputs_keep_float32_autograd_under_the_caps_and_the_recorded_floors(name):
    """The GPU tests allow 4 x what torch's own float32 autograd on the CPU deviates from the float64 stages by.  That
    means something only while the inputs are well conditioned: per tensor below 1e-5 of max|g64| and 1e-6 relative on
    each loss, on every case -- and below the floors recorded in tests/sac_cases.py, which are the worst of these."""
    ec, ep = _float32_deviation(name)
    print("float32 CPU vs float64, %s: critic worst %.2e (%s); policy side worst %.2e (%s)" %
          (name, max(ec.values()), cases.fmt(ec), max(ep.values()), cases.fmt(ep)))
    for k, v in list(ec.items()) + list(ep.items()):
        assert v <= (cases.CAP_LOSS if k.endswith("_loss") else cases.CAP_TENSOR), (name, k, v)
    assert max(ec.values()) <= cases.FLOOR_CRITIC, (name, ec)
    assert max(ep.values()) <= cases.FLOOR_POLICY, (name, ep)


def test_recorded_floors_are_the_worst_case_and_not_above_it():
    """The floors are measurements, not allowances: the worst case comes within a factor 2 of each."""
    worst_c = max(max(_float32_deviation(n)[0].values()) for n in cases.TABLE + cases.EDGE)
    worst_p = max(max(_float32_deviation(n)[1].values()) for n in cases.TABLE + cases.EDGE)
    print("worst float32 deviation: critic %.3e (floor %.1e), policy side %.3e (floor %.1e)" %
          (worst_c, cases.FLOOR_CRITIC, worst_p, cases.FLOOR_POLICY))
    assert cases.FLOOR_CRITIC / 2 <= worst_c <= cases.FLOOR_CRITIC
    assert cases.FLOOR_POLICY / 2 <= worst_p <= cases.FLOOR_POLICY


def _raw_log_std_and_pre_tanh(name):
    """float64, both samples of every update: [(raw log_std, pre-tanh), ...] over (x', eps_next) and (x, eps_pi)"""
    c = cases.case(name)
    pol = R.policy_dict([t.detach().double() for t in cases.split_policy(c, c.sac._pflat)])
    out = []
    for u in range(cases.N_UPDATES):
        b = cases.batch(name, u)
        for x, eps in ((b["x2"], c.eps_next[u]), (b["x"], c.eps_pi[u])):
            _, _, raw, x_t = R.sample(pol, x.double(), eps.double(), c.act_mask.double(), c.log_sig_max)
            out.append((raw, x_t))
    return c, out


@pytest.mark.parametrize("name", cases.TABLE + cases.EDGE)
def test_no_log_std_sits_near_a_clamp_bound(name):
    c, samples = _raw_log_std_and_pre_tanh(name)
    for raw, _ in samples:
        for i, na in enumerate(c.sac.acts):
            r = raw[i, :, :na]
            assert float((r - LOG_SIG_MIN).abs().min()) > 1e-3 and float((r - c.log_sig_max).abs().min()) > 1e-3


def test_edge_cases_take_the_intended_branch():
    c, samples = _raw_log_std_and_pre_tanh("clamped")
    assert c.log_sig_max == -0.5
    for raw, _ in samples:
        for i, na in enumerate(c.sac.acts):
            hi, lo, mid = cases.clamped_columns(na)
            assert len(hi) and len(lo) and (len(mid) or na < 3)
            assert float(raw[i][:, hi].min()) >= c.log_sig_max + 1.0
            assert float(raw[i][:, lo].max()) <= LOG_SIG_MIN - 1.0
            if len(mid):
                assert float(raw[i][:, mid].min()) >= LOG_SIG_MIN + 1.0
                assert float(raw[i][:, mid].max()) <= c.log_sig_max - 1.0
    c, samples = _raw_log_std_and_pre_tanh("saturated")
    for raw, x_t in samples:
        for i, na in enumerate(c.sac.acts):
            up, dn = cases.saturated_columns(na)
            assert len(up)
            assert float(x_t[i][:, up].min()) >= 15.0 and (not len(dn) or float(x_t[i][:, dn].max()) <= -15.0)
            sat = torch.cat([up, dn])
            assert float((raw[i][:, sat].exp() * c.eps_pi[0][i][:, sat].abs()).max()) <= 3.0
            # float32's tanh is exactly +-1 there
            assert bool((torch.tanh(x_t[i][:, sat].float()).abs() == 1.0).all())
            rest = torch.ones(na, dtype=torch.bool)
            rest[sat] = False
            assert float(x_t[i][:, :na][:, rest].abs().max()) < 8.0
    c = cases.case("short_ring")
    assert c.rows == 7 and c.sac.memory.capacity == 64 and int(c.idx.max()) < 7


def test_every_case_has_masked_rows_rewards_of_both_signs_and_an_asymmetric_start():
    for name in cases.TABLE + cases.EDGE:
        c = cases.case(name)
        m, r = c.data["mask"], c.data["reward"]
        assert 0 < float((m == 0).float().mean()) < (0.3 if c.rows > 7 else 0.5)
        assert float(r.min()) < 0 < float(r.max())
        assert c.B == 1 or float(r.abs().max() / r.abs().median()) > 5          # (one row: magnitudes 1 to 3, see case())
        assert torch.equal(c.sac._ctflat, 0.9 * c.sac._cflat)
        q = c.sac.critic
        assert not torch.equal(q[0]["Win"], q[1]["Win"]) and float(q[0]["bin"].detach().abs().min()) > 0
        assert float(c.sac.policy.Wm.abs().max()) > 0
    aligned = lambda c: not (c.H & 3) and not ((2 * c.Na) & 3) and not ((2 * c.Hc) & 3)      # noqa: E731
    assert all(not aligned(cases.case(n)) for n in cases.UNALIGNED)
    assert all(aligned(cases.case(n)) for n in ("aligned", "aligned_gen", "ragged_batch", "fixed_alpha") + cases.EDGE)
    c = cases.case("odd_head")
    assert (c.sac.ins, c.sac.acts) == ([237, 6], [79, 2])
    assert cases.case("aligned").sac.ins == [320, 8] and cases.case("one_row_deep").L == 8


def test_draws_restate_the_documented_streams():
    from oracle import aoref
    seed, step, A, B, Na = 3, 2, 2, 64, 5
    idx, e_next, e_pi = R.draws(seed, step, A, B, Na, rows=7)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (A, B) and tuple(e_pi.shape) == (A, B, Na)
    assert int(idx.min()) >= 0 and int(idx.max()) < 7
    assert sorted(set(idx.reshape(-1).tolist())) == list(range(7))            # every row of a short ring is hit
    for rows in (1, 200, 2 ** 31 + 5):
        i2 = R.draws(seed, step, 1, 8, 1, rows)[0]
        assert int(i2.min()) >= 0 and int(i2.max()) < rows
    # the element mapping, two entries by hand: (a, b) = (1, 5) -> counter step | (1 * 64 + 5) << 32, element j
    assert e_next[1, 5, 3] == aoref.normals(3, 12, 2 | (69 << 32), 4)[3]
    assert e_pi[0, 63, 4] == aoref.normals(3, 13, 2 | (63 << 32), 5)[4]
    x = aoref.philox((69, 2, 0, 11), (3, 0x414F4D52))
    assert int(idx[1, 5]) == (int(x[0]) * 7) >> 32
    # another update, another agent row, another stream: other numbers
    assert not torch.equal(e_next, e_pi) and not torch.equal(R.draws(seed, 3, A, B, Na, 7)[1], e_next)
    assert np.isfinite(e_next.numpy()).all() and 0.8 < float(e_next.std()) < 1.2
