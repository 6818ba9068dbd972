"""Training of the WFS-image denoiser on the GPU: the native step (aomarl_denoiser_trainer_*,
csrc/aomarl_denoise_train.hip) against the float64 autograd statement pinned by test_denoiser_train.py,
its Adam against Adam of its own gradients, determinism, paired recording, and that it trains.

Bounds: per tensor max|g - g64| / max|g64| <= 1e-5 and 5e-7 on the loss = 4x what
torch's own float32 CPU autograd deviates from float64 by on these inputs (checked on the CPU by
test_inputs_of_the_gpu_gradient_test_keep_float32_autograd_below_3e_6); 2.5e-6 on the loss sequence of
twenty steps = 4 x 6e-7 likewise."""
import types

import numpy as np
import pytest
import torch

from ao_marl_amd import denoiser as D
from tests import denoiser_train_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIG = "production_sh_40x40_8m_3layers_d0_noise"


# ------------------------------------------------------------------------------------------ G1
@pytest.mark.parametrize("name", cases.WEIGHTS)
@pytest.mark.parametrize("nimg", cases.NIMG)
def test_g1_gradients_match_float64_autograd(name, nimg):
    tr = D.DenoiserTrainer(cases.weights(name), device=DEV, max_batch=cases.CHUNK)
    assert tr.native
    n, c = cases.pairs(nimg)
    loss, g = tr.grads(n.to(DEV), c.to(DEV))
    l64, g64 = cases.autograd(name, nimg, torch.float64)
    el, eg = cases.grad_errors(loss, g, l64, g64)
    print("G1 %s nimg %d: loss %.3e worst %.3e %s" % (name, nimg, el, max(eg.values()),
                                                      {k: "%.1e" % v for k, v in eg.items()}))
    assert el <= 5e-7, (el, eg)
    assert max(eg.values()) <= 1e-5, eg
    for k in D.PARAM_KEYS:
        assert g[k].shape == g64[k].shape


@pytest.mark.parametrize("name", cases.WEIGHTS)
def test_g1_gradients_at_the_production_sizes(name):
    """max_batch past the cap of 2048 images per pass, three images into a second pass: the 128-wide GEMM tiles and 128
    slabs train_denoiser(batch=4096) runs on.  Same bound as every other G1 case (see cases.big_pairs for the inputs)."""
    tr = D.DenoiserTrainer(cases.weights(name), device=DEV, max_batch=cases.BIG_MAX_BATCH)
    n, c = cases.big_pairs()
    loss, g = tr.grads(n.to(DEV), c.to(DEV))
    l64, g64 = cases.big_autograd(name)
    el, eg = cases.grad_errors(loss, g, l64, g64)
    print("G1 %s nimg %d: loss %.3e worst %.3e %s" % (name, cases.BIG_NIMG, el, max(eg.values()),
                                                      {k: "%.1e" % v for k, v in eg.items()}))
    assert el <= 5e-7, (el, eg)
    assert max(eg.values()) <= 1e-5, eg


def test_native_trainer_refuses_a_non_positive_eps():
    with pytest.raises(ValueError, match="eps"):
        D.DenoiserTrainer(cases.weights("fresh"), device=DEV, eps=0.0)
    from ao_marl_amd import libaomarl as la
    import ctypes as C
    host = {k: v.contiguous().numpy() for k, v in cases.weights("fresh").items()}
    fp = C.POINTER(C.c_float)
    wt = (fp * 6)(*[host[k + ".weight"].ctypes.data_as(fp) for k in D.KEYS])
    bs = (fp * 6)(*[host[k + ".bias"].ctypes.data_as(fp) for k in D.KEYS])
    h = C.c_void_p()
    assert la.load().aomarl_denoiser_trainer_create(wt, bs, 1e-3, 0.9, 0.999, 0.0, 64, C.byref(h)) != 0
    assert not h.value


def test_g1_grads_leaves_the_weights_alone_and_repeats_bit_for_bit():
    tr = D.DenoiserTrainer(cases.weights("fresh"), device=DEV, max_batch=cases.CHUNK)
    n, c = (t.to(DEV) for t in cases.pairs(cases.CHUNK + 3))
    w0 = tr.state_dict()
    l1, g1 = tr.grads(n, c)
    l2, g2 = tr.grads(n, c)
    w1 = tr.state_dict()
    assert torch.equal(l1, l2)
    for k in D.PARAM_KEYS:
        assert torch.equal(g1[k], g2[k]) and torch.equal(w0[k], w1[k])
        assert torch.equal(w0[k].cpu(), cases.weights("fresh")[k])          # the checkpoint's layout, unchanged


# ------------------------------------------------------------------------------------------ G2
@pytest.mark.parametrize("name", cases.WEIGHTS)
def test_g2_update_is_adam_of_the_kernels_own_gradients(name):
    lr, (b1, b2), eps = 1e-3, (0.9, 0.999), 1e-8
    tr = D.DenoiserTrainer(cases.weights(name), lr=lr, betas=(b1, b2), eps=eps, device=DEV, max_batch=cases.CHUNK)
    bn, bc = cases.trajectory_batches()
    m = {k: 0.0 for k in D.PARAM_KEYS}
    v = {k: 0.0 for k in D.PARAM_KEYS}
    for t in (1, 2, 3):
        n, c = bn[t].to(DEV), bc[t].to(DEV)
        w0 = {k: x.cpu().double().numpy() for k, x in tr.state_dict().items()}
        lg, g = tr.grads(n, c)
        ls = tr.step(n, c)
        assert torch.equal(lg, ls)                   # the step reports the loss before its update
        w1 = {k: x.cpu().numpy() for k, x in tr.state_dict().items()}
        worst = 0.0
        for k in D.PARAM_KEYS:
            gk = g[k].cpu().double().numpy()
            m[k] = b1 * m[k] + (1 - b1) * gk
            v[k] = b2 * v[k] + (1 - b2) * gk * gk
            want = w0[k] - (lr / (1 - b1 ** t)) * m[k] / (np.sqrt(v[k]) / np.sqrt(1 - b2 ** t) + eps)
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            err = np.abs(w1[k].astype(np.float64) - want) / ulp
            worst = max(worst, float(err.max()))
            assert float(np.abs(w1[k] - w0[k].astype(np.float32)).max()) > 0, k      # it moved
        print("G2 %s step %d: worst %.2f ulp" % (name, t, worst))
        assert worst <= 2.0, (t, worst)


# ------------------------------------------------------------------------------------------ G3
@pytest.mark.parametrize("name", cases.WEIGHTS)
def test_g3_twenty_steps_follow_float64_and_repeat_bit_for_bit(name):
    bn, bc = (t.to(DEV) for t in cases.trajectory_batches())
    runs = []
    for _ in range(2):
        tr = D.DenoiserTrainer(cases.weights(name), device=DEV, max_batch=cases.CHUNK)
        losses = torch.stack([tr.step(bn[i], bc[i]) for i in range(cases.TRAJ_STEPS)])
        runs.append((losses.cpu(), {k: x.cpu() for k, x in tr.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in D.PARAM_KEYS:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    t64 = cases.trajectory(name, torch.float64)
    dev = [abs(float(a) - b) / abs(b) for a, b in zip(runs[0][0], t64)]
    print("G3 %s: worst relative loss deviation %.3e (%s)" % (name, max(dev), " ".join("%.1e" % d for d in dev)))
    assert max(dev) <= 2.5e-6, dev


# ------------------------------------------------------------------------------------------ G4, G5
NENV, FRAMES = 2, 3


def _supervisor(**kw):
    from ao_marl_amd.env import VecRlSupervisor
    kw.setdefault("prefetch_atmos", False)
    return VecRlSupervisor(CONFIG, {}, NENV, initial_seed=21, **kw)


@pytest.fixture(scope="module")
def recorded():
    """One recording of 8 frames (G4 looks at the first three, G5 trains on six and holds two out), and the
    loop's outputs after frame 3."""
    sup = _supervisor()
    noisy, clean = D.record_pairs(sup, FRAMES)
    after3 = (sup.get_slopes().clone(), sup.get_command().clone(), sup.sim.t["bincube"].clone(),
              sup.sim.t["frame"].clone())
    more = D.record_pairs(sup, 5, reset=False)
    return sup, noisy, clean, after3, more


def test_g4a_recording_does_not_perturb_the_loop(recorded):
    _, noisy, clean, after3, _ = recorded
    sup = _supervisor()
    sup.reset()
    for _ in range(FRAMES):
        sup.next_part_one()
        sup.next_part_two(None, linear_control=True)
    assert torch.equal(sup.get_slopes(), after3[0])
    assert torch.equal(sup.get_command(), after3[1])
    assert torch.equal(sup.sim.t["frame"], after3[3])
    # the sensor image of the frame behind the recorded ones: formed from the same screens, mirrors and noise draws
    sup.sim.next_part_one(write_bincube=True)
    assert noisy.shape == (FRAMES * NENV * sup.s.nvalid, 256) and clean.shape == noisy.shape
    assert torch.equal(sup.sim.t["bincube"].view(-1, 256), recorded[4][0][:NENV * sup.s.nvalid])


def test_g4b_members_are_the_loops_image_and_its_noise_free_formation(recorded):
    _, noisy, clean, _, _ = recorded
    sup = _supervisor()
    sup.reset()
    per = NENV * sup.s.nvalid
    for f in range(FRAMES):
        sup.sim.next_part_one(write_bincube=True)                 # the loop's own frame, cube kept
        assert torch.equal(sup.sim.t["bincube"].view(-1, 256), noisy[f * per:(f + 1) * per]), f
        frame = sup.sim.t["frame"].clone()
        sup.sim.comp_image(noise=False, write_bincube=True, cog=False)
        assert torch.equal(sup.sim.t["bincube"].view(-1, 256), clean[f * per:(f + 1) * per]), f
        sup.sim.t["frame"].copy_(frame)
        sup.iter += 1
        sup.next_part_two(None, linear_control=True)
    assert not torch.equal(noisy, clean)


def test_g4c_noise_is_unbiased(recorded):
    _, noisy, clean, _, _ = recorded
    d = (noisy - clean).double().flatten()
    se = float(d.std()) / d.numel() ** 0.5
    print("G4c: mean %.3e, standard error %.3e, rms %.3f" % (float(d.mean()), se, float(d.std())))
    assert float(d.std()) > 0
    assert abs(float(d.mean())) <= 4 * se


def test_g4d_pipelined_and_prefetched_orders_are_refused(recorded):
    sup = _supervisor(prefetch_atmos=True)
    assert sup.prefetch_atmos
    with pytest.raises(RuntimeError, match="prefetch_atmos"):
        D.record_pairs(sup, 1)
    plain = recorded[0]
    from ao_marl_amd.env import VecAoEnv
    env = VecAoEnv(CONFIG.replace("_d0_", "_d1_"), NENV, initial_seed=21, frame_pipeline=True)   # (the one with norm data)
    assert env.frame_pipeline is True
    with pytest.raises(RuntimeError, match="frame_pipeline"):
        D.record_pairs(env, 1)
    env.frame_pipeline = "auto"
    with pytest.raises(RuntimeError, match="frame_pipeline"):
        D.record_pairs(env, 1)
    # the pipeline switched on underneath a supervisor that is handed over directly
    plain.sim.enable_frame_pipeline()
    try:
        with pytest.raises(RuntimeError, match="frame pipeline is enabled"):
            D.record_pairs(plain, 1)
    finally:
        plain.sim.enable_frame_pipeline(False)
    plain.reset_prefetch = "same"
    try:
        with pytest.raises(RuntimeError, match="reset_prefetch"):
            D.record_pairs(plain, 1)
    finally:
        plain.reset_prefetch = None
    it = plain.iter
    D.record_pairs(types.SimpleNamespace(supervisor=plain, frame_pipeline=False), 1, reset=False, max_pairs=100)
    assert plain.iter == it + 1


def test_g4e_modification_online_is_recorded_in_its_own_order():
    """The reference's recorder runs pure_delay_0 (modification_online): same checks as G4a / G4b in that order."""
    from ao_marl_amd.env import VecRlSupervisor
    sups = [VecRlSupervisor(CONFIG, {"modification_online": True}, NENV, initial_seed=21) for _ in range(2)]
    assert all(s.pure_delay_0 and not s.prefetch_atmos for s in sups)
    noisy, clean = D.record_pairs(sups[0], FRAMES)
    b = sups[1]
    b.reset()
    per = NENV * b.s.nvalid
    for f in range(FRAMES):
        b.next_part_one()
        b.next_part_two(None, linear_control=True)
    assert torch.equal(sups[0].get_slopes(), b.get_slopes())
    assert torch.equal(sups[0].get_command(), b.get_command())
    assert torch.equal(sups[0].sim.t["frame"], b.sim.t["frame"])
    assert torch.equal(sups[0].sim.strehl, b.sim.strehl)
    assert sups[0].iter == b.iter
    b.reset()
    for f in range(FRAMES):
        b._move_or_keep(True)
        frame = b.sim.t["frame"].clone()
        b.sim.comp_image(noise=True, write_bincube=True, cog=False)
        assert torch.equal(b.sim.t["bincube"].view(-1, 256), noisy[f * per:(f + 1) * per]), f
        b.sim.comp_image(noise=False, write_bincube=True, cog=False)
        assert torch.equal(b.sim.t["bincube"].view(-1, 256), clean[f * per:(f + 1) * per]), f
        b.sim.t["frame"].copy_(frame)
        b.sim.comp_image(noise=True, write_bincube=False, cog=True)      # the frame once more, as the loop forms it
        b.sim.do_control()
        b.iter += 1
        b.next_part_two(None, linear_control=True)


def test_record_pairs_returns_per_frame_counts_and_train_denoiser_splits_on_them(recorded):
    sup = recorded[0]
    per = NENV * sup.s.nvalid
    stride = next(s for s in range(5, 60) if 0 < per % s < 3)          # so that the first three offsets differ
    n, c, kept = D.record_pairs(sup, 3, stride=stride, return_counts=True)
    assert kept == [len(range(f % stride, per, stride)) for f in range(3)] and sum(kept) == n.shape[0]
    assert len(set(kept)) > 1                          # the rotating offset: frames keep different numbers
    tr, rep = D.train_denoiser(sup, 2, 2, batch=64, held_out_frames=1, stride=stride)
    assert rep["pairs_per_frame"] == kept and rep["n_train"] == kept[0] + kept[1]      # whole frames, not a proportion
    assert rep["n_train"] != sum(kept) * 2 // 3


def test_record_pairs_subsamples_to_max_pairs(recorded):
    sup = recorded[0]
    per = NENV * sup.s.nvalid
    n, c = D.record_pairs(sup, 2, max_pairs=1000)
    assert n.shape == c.shape and n.shape[1] == 256 and 0 < n.shape[0] <= 1000
    assert n.shape[0] >= 2 * (per // (2 * per // 1000 + 2))


def test_g5_it_trains_on_recorded_frames(recorded):
    sup, noisy3, clean3, _, (noisy5, clean5) = recorded
    per = NENV * sup.s.nvalid
    noisy, clean = torch.cat([noisy3, noisy5]), torch.cat([clean3, clean5])
    ntrain = 6 * per
    tr = D.DenoiserTrainer(None, device=DEV, seed=1, max_batch=256)
    g = torch.Generator(device=DEV).manual_seed(0)
    perm = torch.randperm(ntrain, generator=g, device=DEV)
    for k in range(200):
        idx = perm[(k * 256) % (ntrain - 256):][:256]
        tr.step(noisy[idx], clean[idx])
    hn, hc = noisy[ntrain:], clean[ntrain:]
    held, ident = float(tr.loss(hn, hc)), float(((hn - hc).double() ** 2).mean())
    print("G5: held-out loss %.4f, identity %.4f, ratio %.4f" % (held, ident, held / ident))
    assert held < ident
    cube = hn.view(2, per, 256)[:, :sup.s.nvalid].contiguous()
    want = tr.forward(cube.view(-1, 256)).view_as(cube)
    got = tr.denoiser().denoise_bincube_(cube.clone(), f32=True)
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())


def test_train_denoiser_records_shuffles_and_reports(recorded):
    sup = recorded[0]
    tr, rep = D.train_denoiser(sup, 2, 20, batch=128, held_out_frames=1, seed=2, max_pairs=3000)
    assert tr.native and tr.steps == 20 and rep["train"].shape == (20,)
    assert bool(torch.isfinite(rep["train"]).all()) and float(rep["held_out"]) > 0 and float(rep["identity"]) > 0
    assert float(rep["train"][-5:].mean()) < float(rep["train"][:5].mean())
