"""Inputs shared by the SAC-update conformance tests (test_sac_reference.py on the CPU, test_gpu_sac_update.py on
the GPU): seeded cases -- a BatchedSAC on the CPU whose flat buffers are the parameters, its replay rows, the rows and
normals of three updates -- and the float64 results of tests/sac_reference.py on them.  Everything is computed once per
process and never modified.

Shapes: the smallest at which each path of aomarl_sac_update can go wrong (see CASES).  Conditioning: with unit-variance
states and an unscaled head the pre-tanh value is often several units, 1 - y^2 cancels in float32 and torch's own
float32 autograd is 1e-4 .. 3e-3 off float64 on the head tensors; Wm and Ws are scaled by 0.25 after initialisation,
which keeps it below 1e-5 of max|g64| on every tensor of every case (asserted by test_sac_reference.py, which also
holds every case to the floors recorded below)."""
import functools
import types

import torch

from ao_marl_amd.agents import AgentLayout, LOG_SIG_MIN
from ao_marl_amd.sac import BatchedSAC
from tests import sac_reference as R

# what torch's own float32 autograd on the CPU (BatchedSAC(native=False).update) deviates from the float64 statement by,
# worst over all cases and tensors, measured by test_sac_reference.py (which prints every figure and fails above these):
# per tensor max|g32 - g64| / max|g64|.  FLOOR_CRITIC: the eight critic tensors; FLOOR_POLICY: the policy tensors, the
# temperature gradient, and the relative error of the three losses.  The GPU tests allow 4 x these.
FLOOR_CRITIC = 7.0e-7        # measured 5.84e-7 (odd_critic, Wout of Q2)
FLOOR_POLICY = 5.5e-7        # measured 4.29e-7 (odd_hidden, Wh1); losses <= 2.4e-7, temperature gradient <= 9.8e-8
FACTOR = 4.0
# the conditioning caps: a case above them gets other inputs, never a looser cap
CAP_TENSOR, CAP_LOSS = 1e-5, 1e-6

N_UPDATES = 3
ROWS = 200


def _layout(which):
    if which == "LA":       # ins [320, 8], acts [80, 2]
        return AgentLayout(87, [0, 80], 1, include_tip_tilt=True, n_filtered=5)
    # ins [237, 6], acts [79, 2]: in_max and in_max + act_max ragged, 2 act_max = 158 not a multiple of 4
    return AgentLayout(87, [0, 79], 1, include_tip_tilt=True, n_filtered=5,
                       state_keys=("dm_history_1", "dm_before_linear", "dm_residual"))


_FIXED = dict(automatic_entropy_tuning=False, alpha=0.3, target_update_interval=2, gamma=0.5)
# name: (layout, actor layers, H, Hc, B, extra configuration, edge)
CASES = {
    "aligned": ("LA", 2, 64, 64, 64, {}, None),            # k_gemm_g_multi: the production code path in small
    "aligned_gen": ("LA", 2, 64, 64, 64, {}, None),        # the same under AOMARL_SAC_GEMM=gen
    "ragged_batch": ("LA", 1, 68, 36, 37, {}, None),       # partial wave groups, second pass of the row-group loops
    "odd_head": ("LB", 3, 64, 32, 33, {}, None),           # unaligned through 2 act_max; ragged I and NA; three layers
    "odd_hidden": ("LA", 2, 30, 18, 5, {}, None),          # unaligned through H; B < 32
    "odd_critic": ("LA", 2, 32, 33, 64, {}, None),         # unaligned through 2 Hc = 66; ragged column block
    "one_row_deep": ("LB", 8, 16, 16, 1, {}, None),        # B = 1; SAC_MAX_HIDDEN layers
    "fixed_alpha": ("LA", 2, 64, 64, 64, _FIXED, None),    # no soft update on odd steps, temperature untouched
    # edge values, on the aligned shape, far from every decision boundary
    "clamped": ("LA", 2, 64, 64, 64, dict(LOG_SIG_MAX=-0.5), "clamped"),
    "saturated": ("LA", 2, 64, 64, 64, {}, "saturated"),
    "short_ring": ("LA", 2, 64, 64, 64, {}, "short_ring"),
}
TABLE = tuple(k for k, v in CASES.items() if v[6] is None)
EDGE = tuple(k for k, v in CASES.items() if v[6] is not None)
UNALIGNED = ("odd_head", "odd_hidden", "odd_critic")       # aomarl_sac_create: aligned == false
SHORT_ROWS, SHORT_CAPACITY = 7, 64
# one_row_deep is ONE row: each loss is one squared difference, every gradient one outer product, and float32 keeps them
# to the caps only where nothing cancels; of twelve seeds tried, five kept every figure below 6e-7, this is one of them
SEEDS = {"one_row_deep": 2002}


def clamped_columns(na):
    """(above LOG_SIG_MAX, below LOG_SIG_MIN, inside) column indices of an agent with na real action columns."""
    j = torch.arange(na)
    return j[j % 3 == 0], j[j % 3 == 1], j[j % 3 == 2]


def saturated_columns(na):
    """(bm = +20, bm = -20) column indices"""
    j = torch.arange(na)
    return j[j % 8 == 0], j[j % 8 == 4]


def new_sac(name, device="cpu", native=False):
    """A BatchedSAC of the case's configuration (its own initialisation: the case's parameters are copied in)."""
    lay, L, H, Hc, B, extra, edge = CASES[name]
    cfg = dict(num_layers_actor=L, hidden_size_actor=H, hidden_size_critic=Hc, batch_size=B,
               initialize_last_layer_0=False, memory_size=SHORT_CAPACITY if edge == "short_ring" else ROWS)
    cfg.update(extra)
    return BatchedSAC(_layout(lay), cfg, seed=3, device=device, native=native)


@functools.lru_cache(maxsize=None)
def case(name):
    lay, L, H, Hc, B, extra, edge = CASES[name]
    sac = new_sac(name)
    A, Na = sac.A, sac.act_max
    g = torch.Generator().manual_seed(SEEDS.get(name, 1000 + sorted(CASES).index(name.replace("_gen", ""))))
    p = sac.policy

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    with torch.no_grad():
        # off the symmetric start: every real weight moved, biases non-zero, the two critics apart, the target its own
        sac._pflat.add_(0.02 * rn(sac._pflat.numel()) * (sac._pflat != 0))
        sac._cflat.add_(0.02 * rn(sac._cflat.numel()) * (sac._cflat != 0))
        p.Wm.mul_(0.25); p.Ws.mul_(0.25)                              # conditioning (module docstring)
        for b in [p.b1] + list(p.bh):
            b.copy_(0.05 * rn(*b.shape))
        p.bm.copy_(0.05 * rn(*p.bm.shape) * sac.act_mask)
        p.bs.copy_((0.05 * rn(*p.bs.shape) - 1.0) * sac.act_mask)
        for k, q in enumerate(sac.critic):
            q["bin"].copy_(0.05 * rn(*q["bin"].shape))
            q["bout"].fill_(0.1 * (k + 1))
        if edge == "clamped":
            for i, na in enumerate(sac.acts):
                hi, lo, mid = clamped_columns(na)
                p.bs[i, 0, hi] = sac.policy.log_sig_max + 3.0
                p.bs[i, 0, lo] = LOG_SIG_MIN - 5.0
                p.bs[i, 0, mid] = -6.0
        if edge == "saturated":
            for i, na in enumerate(sac.acts):
                up, dn = saturated_columns(na)
                p.bm[i, 0, up], p.bm[i, 0, dn] = 20.0, -20.0
        sac._ctflat.copy_(0.9 * sac._cflat)
        sac.log_alpha.copy_(0.1 * rn(A, 1, 1))                        # (alpha keeps the configured start)
    rows = SHORT_ROWS if edge == "short_ring" else ROWS
    sd, ad = sac.layout.state_dim, sac.layout.action_dim
    data = dict(state=rn(rows, sd), action=torch.rand(rows, ad, generator=g) * 2 - 1,
                # both signs, magnitudes from 0.03 to 3
                reward=rn(rows, A) * 10.0 ** (torch.rand(rows, A, generator=g) * 2 - 1.5),
                next_state=rn(rows, sd), mask=(torch.rand(rows, generator=g) > 0.1).float())
    if B == 1:
        # a single row: each loss is ONE squared difference q - target, which float32 keeps to 1e-6 only while the two
        # are well apart -- rewards of magnitude 1 to 3 (q is a few tenths), still of both signs
        data["reward"] = torch.sign(data["reward"]) * (1.0 + 2.0 * torch.rand(rows, A, generator=g))
    if edge == "short_ring":
        data["mask"][2] = 0.0
    idx = torch.randint(0, rows, (N_UPDATES, A, B), generator=g)
    eps_next, eps_pi = rn(N_UPDATES, A, B, Na), rn(N_UPDATES, A, B, Na)
    if edge == "saturated":           # |std eps| <= 3 on the saturated columns (std < 1): tanhf is exactly +-1
        for i, na in enumerate(sac.acts):
            cols = torch.cat(saturated_columns(na))
            for e in (eps_next, eps_pi):
                e[:, i, :, cols] = e[:, i, :, cols].clamp(-3.0, 3.0)
    return types.SimpleNamespace(name=name, sac=sac, A=A, B=B, L=L, H=H, Hc=Hc, I=sac.in_max, Na=Na, rows=rows,
                                 edge=edge, data=data, idx=idx, eps_next=eps_next.contiguous(),
                                 eps_pi=eps_pi.contiguous(), log_sig_max=float(p.log_sig_max), gamma=float(sac.gamma),
                                 act_mask=sac.act_mask.clone(), alpha=sac.alpha.detach().clone(),
                                 target_entropy=sac.target_entropy.clone())


# ------------------------------------------------------------------------------------ flat buffers <-> tensors
def _view(flat, off, *shape):
    n = 1
    for k in shape:
        n *= k
    return flat[off:off + n].view(*shape)


def split_policy(c, flat):
    """A flat policy-shaped buffer (parameters, gradients, moments) cut into R.policy_list order."""
    A, I, Na, H, L, po = c.A, c.I, c.Na, c.H, c.L, c.sac._poff
    head, bhead = _view(flat, po[2 * L], A, H, 2 * Na), _view(flat, po[2 * L + 1], A, 1, 2 * Na)
    return [_view(flat, po[0], A, I, H), _view(flat, po[1], A, 1, H)] + \
        [_view(flat, po[2 * l], A, H, H) for l in range(1, L)] + \
        [_view(flat, po[2 * l + 1], A, 1, H) for l in range(1, L)] + \
        [head[:, :, :Na], bhead[:, :, :Na], head[:, :, Na:], bhead[:, :, Na:]]


def split_critic(c, flat):
    """A flat critic-shaped buffer cut into the two critics' dicts."""
    A, I, Na, Hc, co = c.A, c.I, c.Na, c.Hc, c.sac._coff
    win, bin_ = _view(flat, co[0], A, I + Na, 2 * Hc), _view(flat, co[1], A, 1, 2 * Hc)
    wout, bout = _view(flat, co[2], A, 2, Hc), _view(flat, co[3], A, 2)
    return [dict(Win=win[:, :, k * Hc:(k + 1) * Hc], bin=bin_[:, :, k * Hc:(k + 1) * Hc],
                 Wout=wout[:, k, :].unsqueeze(2), bout=bout[:, k].reshape(A, 1, 1)) for k in range(2)]


POLICY_NAMES = lambda L: (["W1", "b1"] + ["Wh%d" % l for l in range(1, L)] + ["bh%d" % l for l in range(1, L)] +  # noqa: E731
                          ["Wm", "bm", "Ws", "bs"])


def gather_batch(c, idx, data=None):
    """Replay rows idx [A, B] split per agent as the update reads them (its own statement of the gather: state entries
    modes_chosen[i], action columns action_slices[i], reward column i; padding zero)."""
    data = data or c.data
    lay = c.sac.layout
    x, x2 = torch.zeros(c.A, c.B, c.I), torch.zeros(c.A, c.B, c.I)
    a = torch.zeros(c.A, c.B, c.Na)
    r, mask = torch.zeros(c.A, c.B, 1), torch.zeros(c.A, c.B, 1)
    for i, (sel, (lo, hi)) in enumerate(zip(lay.modes_chosen.values(), lay.action_slices.values())):
        sel = torch.as_tensor(sel, dtype=torch.long)
        rows = idx[i]
        x[i, :, :len(sel)] = data["state"][rows][:, sel]
        x2[i, :, :len(sel)] = data["next_state"][rows][:, sel]
        a[i, :, :hi - lo] = data["action"][rows][:, lo:hi]
        r[i, :, 0], mask[i, :, 0] = data["reward"][rows, i], data["mask"][rows]
    return dict(x=x, a=a, r=r, x2=x2, mask=mask)


# ------------------------------------------------------------------------------------ references
def critic_reference_at(c, policy, critic, critic_target, alpha, batch, eps_next):
    return R.critic_stage(policy, critic, critic_target, alpha, batch, eps_next, c.gamma, c.act_mask, c.log_sig_max)


def actor_reference_at(c, policy, critic_after, alpha, batch, eps_pi):
    return R.actor_stage(policy, critic_after, alpha, batch, eps_pi, c.act_mask, c.log_sig_max)


@functools.lru_cache(maxsize=None)
def batch(name, u=0):
    c = case(name)
    return gather_batch(c, c.idx[u])


@functools.lru_cache(maxsize=None)
def critic_reference(name):
    """float64 critic stage of update 1 on the case's parameters."""
    c = case(name)
    return critic_reference_at(c, R.policy_dict(split_policy(c, c.sac._pflat)), split_critic(c, c.sac._cflat),
                               split_critic(c, c.sac._ctflat), c.alpha, batch(name), c.eps_next[0])


def actor_reference(name, critic_after_flat):
    """float64 actor stage of update 1 on the case's policy and the given critic (a flat buffer read back)."""
    c = case(name)
    return actor_reference_at(c, R.policy_dict(split_policy(c, c.sac._pflat)), split_critic(c, critic_after_flat),
                              c.alpha, batch(name), c.eps_pi[0])


@functools.lru_cache(maxsize=None)
def float32_statement(name):
    """torch's float32 autograd of update 1 on the CPU (BatchedSAC(native=False).update with keep_grads):
    dict(critic grads, policy grads, la_grad, losses, critic_after flat)."""
    c = case(name)
    s = new_sac(name)
    with torch.no_grad():
        s._pflat.copy_(c.sac._pflat); s._cflat.copy_(c.sac._cflat); s._ctflat.copy_(c.sac._ctflat)
        s.log_alpha.copy_(c.sac.log_alpha); s.alpha.copy_(c.sac.alpha)
    s.keep_grads = True
    b = batch(name)
    losses = s.update(b["x"], b["a"], b["r"], b["x2"], b["mask"], eps_next=c.eps_next[0], eps_pi=c.eps_pi[0])
    la = s.grad_log["log_alpha"].reshape(-1) if s.automatic_entropy_tuning else None
    return dict(critic=s.grad_log["critic"], policy=s.grad_log["policy"], la_grad=la,
                losses={k: v.detach().reshape(-1) for k, v in losses.items()},
                critic_after=s._cflat.detach().clone())


# ------------------------------------------------------------------------------------ metrics
def tensor_error(got, want):
    """max|g - g64| / max|g64|"""
    want = want.double()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def relative_error(got, want):
    """worst relative error over the agents"""
    want = want.double().reshape(-1)
    return float(((got.detach().double().cpu().reshape(-1) - want).abs() / want.abs()).max())


def stage_errors(c, cgrads, pgrads, la_grad, losses, cref, aref):
    """Deviations of one update's outputs from the float64 stages: (critic {name: error}, policy-side {name: error}).
    cgrads: the two critics' dicts; pgrads: policy_list order; la_grad [A] or None; losses: q1, q2, policy [A]."""
    ec = {"%s%d" % (k, q + 1): tensor_error(cgrads[q][k], cref["grads"][k][q]) for k in R.CRITIC_KEYS for q in range(2)}
    ep = {n: tensor_error(g, w) for n, g, w in zip(POLICY_NAMES(c.L), pgrads, aref["grads"])}
    if la_grad is not None:
        ep["la_grad"] = tensor_error(la_grad.reshape(-1), R.alpha_grad(aref["mean_log_pi"], c.target_entropy))
    ep["q1_loss"] = relative_error(losses["q1"], cref["q1_loss"])
    ep["q2_loss"] = relative_error(losses["q2"], cref["q2_loss"])
    ep["policy_loss"] = relative_error(losses["policy"], aref["policy_loss"])
    return ec, ep


def fmt(errors):
    return " ".join("%s %.1e" % kv for kv in errors.items())
