#!/usr/bin/env python3
"""Golden vector for the denoiser's training step, produced by running the reference's own module
(build container only): 8 noisy / clean spot pairs, the MSE loss of
DenoisingAutoencoderCNN2DSingleSubapeture (src/autoencoder/autoencoder_models.py:130-197) on the
shipped weights and its float64 autograd gradients of all 12 tensors.
Writes tests/golden/host_denoiser_train.pt (data only).  The pairs are stored as this repo's
[y][x] tiles; the module is fed their transposes, as the reference feeds it.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _ref_shims  # noqa: E402

import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def main():
    from src.autoencoder.autoencoder_models import DenoisingAutoencoderCNN2DSingleSubapeture
    from ao_marl_amd.denoiser import shipped_weights_path, synthetic_pairs
    sd = torch.load(shipped_weights_path(), map_location="cpu", weights_only=True)
    sd = sd.get("state_dict", sd)
    m = DenoisingAutoencoderCNN2DSingleSubapeture().double()
    m.load_state_dict({k: v.double() for k, v in sd.items()})
    noisy, clean = synthetic_pairs(8, seed=11)
    x = noisy.double().view(-1, 16, 16).transpose(1, 2).unsqueeze(1)
    y = clean.double().view(-1, 16, 16).transpose(1, 2).unsqueeze(1)
    loss = torch.nn.MSELoss()(m(x), y)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    torch.save({"noisy": noisy, "clean": clean, "loss": loss.detach().clone(), "grads": grads},
               os.path.join(OUT, "host_denoiser_train.pt"))
    print("denoiser train", float(loss), {k: float(v.abs().max()) for k, v in grads.items()})


if __name__ == "__main__":
    _ref_shims.install()
    os.makedirs(OUT, exist_ok=True)
    main()
