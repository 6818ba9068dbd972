"""Training of the WFS-image denoiser, CPU side: the autograd statement of the step
(ao_marl_amd.denoiser.DenoiserTrainer(native=False)) against the reference module's own autograd
(golden fixture, tools/gen_golden_denoiser_train.py), its Adam against torch.optim.Adam, the
checkpoint round trip, and the condition on the inputs the GPU tests' bounds rest on."""
import os

import pytest
import torch

from ao_marl_amd import denoiser as D
from tests import denoiser_train_cases as cases


def test_c1_autograd_statement_matches_the_reference_modules_autograd():
    """Loss and the float64 gradients of all 12 tensors on the shipped weights == what the reference's
    DenoisingAutoencoderCNN2DSingleSubapeture + MSELoss gave (sigmoid branch off), to 1e-10."""
    fx = cases.fixture()
    tr = D.DenoiserTrainer(cases.weights("shipped"), native=False, device="cpu", dtype=torch.float64)
    loss, g = tr.grads(fx["noisy"], fx["clean"])
    assert abs(float(loss) - float(fx["loss"])) <= 1e-10 * abs(float(fx["loss"]))
    assert set(fx["grads"]) == set(D.PARAM_KEYS)
    for k in D.PARAM_KEYS:
        ref = fx["grads"][k]
        assert g[k].shape == ref.shape and ref.dtype == torch.float64
        assert float((g[k] - ref).abs().max()) <= 1e-10 * float(ref.abs().max()), k


def test_c2_three_steps_equal_torch_optim_adam():
    n, c = cases.pairs(37)
    tr = D.DenoiserTrainer(cases.weights("fresh"), native=False, device="cpu", dtype=torch.float64,
                           lr=2e-3, betas=(0.8, 0.95), eps=1e-7)
    w = {k: v.detach().double().clone().requires_grad_(True) for k, v in cases.weights("fresh").items()}
    opt = torch.optim.Adam([w[k] for k in D.PARAM_KEYS], lr=2e-3, betas=(0.8, 0.95), eps=1e-7)
    for step in range(3):
        x, y = n[step:step + 30], c[step:step + 30]
        loss = tr.step(x, y)
        opt.zero_grad()
        ref = ((D.net_forward(w, D._tiles_to_net(x.double())) - D._tiles_to_net(y.double())) ** 2).mean()
        ref.backward()
        opt.step()
        assert abs(float(loss) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
        sd = tr.state_dict()
        for k in D.PARAM_KEYS:
            assert float((sd[k] - w[k].detach()).abs().max()) <= 1e-12 * float(w[k].detach().abs().max()), (step, k)
    assert tr.steps == 3


def test_c3_save_load_round_trip_is_bit_exact(tmp_path):
    n, c = cases.pairs(37)
    tr = D.DenoiserTrainer(None, native=False, device="cpu", seed=4)
    for _ in range(2):
        tr.step(n, c)
    path = os.path.join(str(tmp_path), "dn.pt")
    tr.save(path)
    a, b = tr.denoiser(device="cpu"), D.SubapDenoiser.load(path, device="cpu")
    cube = n.view(1, -1, 256).clone()
    assert torch.equal(a.denoise_bincube_(cube.clone()), b.denoise_bincube_(cube.clone()))
    want = tr.forward(n)                   # the trainer's own statement of the forward (another memory format)
    assert float((b.denoise_bincube_(cube.clone()).view(-1, 256) - want).abs().max()) <= 2e-5 * float(want.abs().max())


def test_fresh_initialisation_is_seeded_and_leaves_the_global_generator_alone():
    torch.manual_seed(99)
    before = torch.random.get_rng_state()
    a, b, c = D.fresh_state_dict(1), D.fresh_state_dict(1), D.fresh_state_dict(2)
    assert torch.equal(before, torch.random.get_rng_state())
    assert all(torch.equal(a[k], b[k]) for k in D.PARAM_KEYS)
    assert not torch.equal(a["encoder3.weight"], c["encoder3.weight"])
    fan = {"encoder1": 9, "encoder2": 144, "encoder3": 288, "decoder1": 512, "decoder2": 256, "decoder3": 9}
    for k in D.KEYS:                       # torch's default: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
        assert float(a[k + ".weight"].abs().max()) <= fan[k] ** -0.5
        assert float(a[k + ".weight"].abs().max()) > 0.8 * fan[k] ** -0.5 or a[k + ".weight"].numel() < 200


def test_trainer_refuses_other_layer_shapes_and_native_on_the_cpu():
    sd = dict(cases.weights("fresh"))
    sd["encoder2.weight"] = torch.zeros(32, 16, 5, 5)
    with pytest.raises(ValueError):
        D.DenoiserTrainer(sd, native=False, device="cpu")
    with pytest.raises(ValueError):
        D.DenoiserTrainer(cases.weights("fresh"), native=True, device="cpu")


@pytest.mark.parametrize("name", cases.WEIGHTS)
def test_inputs_of_the_gpu_gradient_test_keep_float32_autograd_below_3e_6(name):
    """The GPU tests allow 1e-5 per tensor, 4x what torch's own float32 autograd deviates from float64 by.
    That only means something while no pre-activation sits within round-off of zero on these inputs (a
    flipped ReLU moves one image's whole contribution): float32 autograd itself must stay below 3e-6, and
    5e-7 on the loss."""
    for nimg in cases.NIMG:
        l64, g64 = cases.autograd(name, nimg, torch.float64)
        l32, g32 = cases.autograd(name, nimg, torch.float32)
        el, eg = cases.grad_errors(l32, g32, l64, g64)
        assert el < 1.25e-7 and max(eg.values()) < 3e-6, (name, nimg, el, eg)
    # the large case repeats these images; its last, partial repeat alone
    l64, g64 = cases._autograd_on(name, *cases.big_tail(), torch.float64)
    l32, g32 = cases._autograd_on(name, *cases.big_tail(), torch.float32)
    el, eg = cases.grad_errors(l32, g32, l64, g64)
    assert el < 1.25e-7 and max(eg.values()) < 3e-6, (name, "tail", el, eg)


def test_reference_of_the_large_case_is_the_weighted_mean_of_its_repeats():
    """big_autograd on a shorter stand-in of the same construction == float64 autograd on the repeated images."""
    n, c = cases.pairs(cases.CHUNK + 3)
    period, nimg = n.shape[0], 2 * n.shape[0] + 5
    idx = torch.arange(nimg) % period
    l, g = cases._autograd_on("fresh", n[idx], c[idx], torch.float64)
    la, ga = cases.autograd("fresh", period, torch.float64)
    lb, gb = cases._autograd_on("fresh", n[:5], c[:5], torch.float64)
    wa, wb = 2 * period / nimg, 5 / nimg
    assert abs(float(wa * la + wb * lb) - float(l)) <= 1e-12 * float(l)
    for k in D.PARAM_KEYS:
        assert float((wa * ga[k] + wb * gb[k] - g[k]).abs().max()) <= 1e-12 * float(g[k].abs().max()), k


def test_trainer_refuses_a_non_positive_eps():
    for eps in (0.0, -1e-8, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            D.DenoiserTrainer(cases.weights("fresh"), native=False, device="cpu", eps=eps)


@pytest.mark.parametrize("name", cases.WEIGHTS)
def test_inputs_of_the_gpu_trajectory_test_keep_float32_autograd_within_6e_7(name):
    t64, t32 = cases.trajectory(name, torch.float64), cases.trajectory(name, torch.float32)
    worst = max(abs(a - b) / abs(b) for a, b in zip(t32, t64))
    assert worst < 6.25e-7, (name, worst)
    assert t64[-1] < t64[0]
