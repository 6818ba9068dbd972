"""Inputs shared by the denoiser-training tests (test_denoiser_train.py on the CPU,
test_gpu_denoiser_train.py on the GPU): seeded synthetic spot pairs plus the 8 pairs of the golden
fixture, the shipped weights and a fresh initialisation, and float64 / float32 autograd on them.
References are computed once per process and never modified."""
import functools
import os

import torch

from ao_marl_amd import denoiser as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 64                    # max_batch of the trainers under test: the workspace holds 64 images
NIMG = (1, 37, 64, CHUNK + 3)   # one image; a partial slab; the whole workspace; three images into a second pass
# the production sizes: a trainer whose max_batch is past the library's cap of 2048 images per pass, on three images
# more than one pass holds (the 128-wide GEMM tiles, 128 split-K slabs, a second pass of one partial slab)
BIG_MAX_BATCH, BIG_NIMG = 4096, 2048 + 3
WEIGHTS = ("shipped", "fresh")
PAIR_SEED, INIT_SEED = 5, 3
TRAJ_STEPS, TRAJ_BATCH, TRAJ_SEED = 20, 64, 17


@functools.lru_cache(maxsize=None)
def fixture():
    return torch.load(os.path.join(GOLDEN, "host_denoiser_train.pt"), weights_only=True)


@functools.lru_cache(maxsize=None)
def weights(name):
    if name == "shipped":
        sd = torch.load(D.shipped_weights_path(), map_location="cpu", weights_only=True)
        return sd.get("state_dict", sd)
    return D.fresh_state_dict(INIT_SEED)


@functools.lru_cache(maxsize=None)
def pairs(nimg):
    """The 8 fixture pairs in front of seeded synthetic ones (a single image: synthetic)."""
    if nimg <= 8:
        return D.synthetic_pairs(nimg, seed=PAIR_SEED)
    n, c = D.synthetic_pairs(nimg - 8, seed=PAIR_SEED)
    fx = fixture()
    return torch.cat([fx["noisy"], n]).contiguous(), torch.cat([fx["clean"], c]).contiguous()


@functools.lru_cache(maxsize=None)
def autograd(name, nimg, dtype):
    """(loss, grads) of the autograd statement on the CPU, as float64 tensors."""
    tr = D.DenoiserTrainer(weights(name), native=False, device="cpu", dtype=dtype)
    loss, g = tr.grads(*pairs(nimg))
    return loss.double(), {k: v.double() for k, v in g.items()}


def _autograd_on(name, noisy, clean, dtype):
    tr = D.DenoiserTrainer(weights(name), native=False, device="cpu", dtype=dtype)
    loss, g = tr.grads(noisy, clean)
    return loss.double(), {k: v.double() for k, v in g.items()}


@functools.lru_cache(maxsize=None)
def big_pairs():
    """BIG_NIMG pairs: the CHUNK + 3 pairs of `pairs`, over and over.  Among thousands of distinct images some
    pre-activation always sits within float32 round-off of zero (torch's own float32 autograd is then 1e-4 off float64
    on one tensor: a flipped ReLU moves an image's whole contribution), and no bound on a differently ordered sum
    holds.  Repeats of images that are known to be free of that (the CPU test of the inputs) keep the large case as
    well conditioned as the small ones; the period, 67, is odd, so every image meets every position of a slab."""
    n, c = pairs(CHUNK + 3)
    idx = torch.arange(BIG_NIMG) % n.shape[0]
    return n[idx].contiguous(), c[idx].contiguous()


@functools.lru_cache(maxsize=None)
def big_tail():
    """The pairs of the last, partial repeat."""
    n, c = pairs(CHUNK + 3)
    r = BIG_NIMG % n.shape[0]
    return n[:r].contiguous(), c[:r].contiguous()


@functools.lru_cache(maxsize=None)
def big_autograd(name, dtype=torch.float64):
    """(loss, grads) of the autograd statement on big_pairs(): the mean over whole repeats and the partial one is the
    weighted mean of the two (exact; in float64 to round-off)."""
    period = CHUNK + 3
    q, r = divmod(BIG_NIMG, period)
    la, ga = autograd(name, period, dtype)
    lb, gb = _autograd_on(name, *big_tail(), dtype)
    wa, wb = q * period / BIG_NIMG, r / BIG_NIMG
    return wa * la + wb * lb, {k: wa * ga[k] + wb * gb[k] for k in D.PARAM_KEYS}


def grad_errors(loss, grads, ref_loss, ref_grads):
    """(relative loss error, {key: max|g - g64| / max|g64|})"""
    el = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    eg = {k: float((grads[k].double().cpu() - ref_grads[k]).abs().max() / ref_grads[k].abs().max())
          for k in D.PARAM_KEYS}
    return el, eg


@functools.lru_cache(maxsize=None)
def trajectory_batches():
    n, c = D.synthetic_pairs(TRAJ_STEPS * TRAJ_BATCH, seed=TRAJ_SEED)
    return n.view(TRAJ_STEPS, TRAJ_BATCH, 256), c.view(TRAJ_STEPS, TRAJ_BATCH, 256)


@functools.lru_cache(maxsize=None)
def trajectory(name, dtype):
    """The loss sequence of TRAJ_STEPS Adam steps of the autograd statement on the CPU."""
    tr = D.DenoiserTrainer(weights(name), native=False, device="cpu", dtype=dtype)
    n, c = trajectory_batches()
    return [float(tr.step(n[i], c[i])) for i in range(TRAJ_STEPS)]
