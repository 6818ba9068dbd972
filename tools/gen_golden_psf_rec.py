#!/usr/bin/env python3
"""The reference's OWN psf_rec_vii_cpu (guardians/gamora.py:103-171), unmodified, on two small synthetic ROKET files
-> tests/golden/psf_rec_vii.npz: the inputs (spup, IF CSR, TT, P, Btt, contributor buffers, lambda) and the reference's
outputs (otftel, otf2, psf).

Build container only (needs the reference tree).  The file is a dict-backed stand-in for h5py.File with
.attrs["_Param_target__Lambda"]; gamora.py and drax.py import h5py, a carmaWrap context instance and sutraWrap's Gamora at
module level, which get stand-ins here (tools/_ref_shims.py stays as the other generators use it).

    case  p   N    obstruction  actuators  modes  frames
    A     24  64   0.14         18         16     48
    B     33  128  none         32         30     90
Influence functions: Gaussians truncated so that a pixel is under at most 16 of them (one lit pixel under none).

Usage: python tools/gen_golden_psf_rec.py
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
os.environ.setdefault("MPLBACKEND", "Agg")
import _ref_shims  # noqa: E402

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

CONTRIBUTORS = ("noise", "aliasing", "tomography", "filtered modes", "non linearity", "bandwidth")
CASES = {"A": dict(p=24, N=64, cobs=0.14, grid=(4, 4), nframes=48, seed=11),
         "B": dict(p=33, N=128, cobs=0.0, grid=(6, 5), nframes=90, seed=12)}
FILES = {}


class _Dataset(object):
    """f[name][:] hands out a copy, as h5py does (drax.get_err adds into what it read)"""

    def __init__(self, a):
        self.a = np.asarray(a)

    def __getitem__(self, k):
        return np.array(self.a[k])

    @property
    def shape(self):
        return self.a.shape


class _File(object):
    def __init__(self, name, mode="r"):
        self.d = FILES[name]
        self.attrs = self.d["attrs"]

    def __getitem__(self, k):
        return _Dataset(self.d["data"][k])

    def keys(self):
        return list(self.d["data"].keys())

    def close(self):
        pass


def install_stand_ins():
    _ref_shims.install()
    h5 = types.ModuleType("h5py")
    h5.File = _File
    sys.modules["h5py"] = h5
    cw = types.ModuleType("carmaWrap")

    class context(object):
        active_device = 0

        @classmethod
        def get_instance_ngpu(cls, n, devices):
            return cls()

    cw.context = context
    sys.modules["carmaWrap"] = cw
    sw = types.ModuleType("sutraWrap")

    class Gamora(object):
        def __init__(self, *a, **k):
            raise RuntimeError("COMPASS's Gamora is not available: only psf_rec_vii_cpu runs here")

    sw.Gamora = Gamora
    sys.modules["sutraWrap"] = sw


def make_case(p, N, cobs, grid, nframes, seed, amplitude):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:p, :p] - (p - 1) / 2.0
    r = np.hypot(x, y) / (p / 2.0)
    spup = ((r <= 1.0) & (r >= cobs)).astype(np.float32)
    lit = np.nonzero(spup)
    npts = lit[0].size
    gy, gx = grid
    ay, ax = np.meshgrid(np.linspace(-0.8, 0.8, gy) * p / 2, np.linspace(-0.8, 0.8, gx) * p / 2, indexing="ij")
    ay, ax = ay.ravel(), ax.ravel()
    nact = ay.size
    pitch = 1.6 * (p / 2) / (max(gy, gx) - 1)
    d2 = (y[lit][None, :] - ay[:, None]) ** 2 + (x[lit][None, :] - ax[:, None]) ** 2       # [nact][npts]
    infl = np.exp(-d2 / (0.7 * pitch) ** 2)
    # the 16 nearest influence functions of every pixel, inside the truncation radius
    radius = 2.6 * pitch
    keep = d2 <= radius ** 2
    order = np.argsort(d2, axis=0)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(nact)[:, None].repeat(npts, 1), axis=0)
    keep &= rank < 16
    keep[:, 0] = False                                                   # one lit pixel under no influence function
    IF = sp.csr_matrix(np.where(keep, infl, 0.0).astype(np.float32))
    taps = np.asarray((IF != 0).sum(axis=0)).ravel()
    assert taps.max() == 16 and taps.min() == 0, (taps.max(), taps.min())
    TT = np.stack([x[lit], y[lit]], axis=1).astype(np.float32) / (p / 2.0)
    nactu, nmodes = nact + 2, nact
    Q, _ = np.linalg.qr(rng.normal(size=(nactu, nmodes)))
    Btt = Q * rng.uniform(0.5, 1.5, size=nmodes)
    P = np.linalg.pinv(Btt)
    data = {"spup": spup, "IF.data": IF.data, "IF.indices": IF.indices, "IF.indptr": IF.indptr, "TT": TT, "P": P, "Btt": Btt}
    for i, n in enumerate(CONTRIBUTORS):
        w = rng.normal(size=(nactu, nframes))
        for t in range(1, nframes):                                       # some temporal correlation
            w[:, t] = 0.6 * w[:, t - 1] + 0.8 * w[:, t]
        data[n] = amplitude * (0.3 + 0.2 * i) * w
    data["zeta_com"] = np.zeros((nactu, nframes))
    assert fft_size_rule(p) == N
    return data


def fft_size_rule(p):
    return 2 ** int(np.log(2 * p) / np.log(2) + 1)


def main():
    install_stand_ins()
    from guardians import gamora
    out = {}
    for name, c in sorted(CASES.items()):
        amplitude = 0.02
        for _ in range(40):
            FILES[name] = dict(data=make_case(amplitude=amplitude, **c), attrs={"_Param_target__Lambda": np.array([1.65])})
            otftel, otf2, psf = gamora.psf_rec_vii_cpu(name)
            sr = float(psf.max())
            if 0.5 <= sr <= 0.9:
                break
            amplitude *= 0.7 if sr < 0.5 else 1.3
        assert 0.3 <= sr <= 0.99, sr
        assert np.isrealobj(otf2) and otf2.shape == (c["N"], c["N"])
        print("case %s: N = %d, %d lit pixels, amplitude %.4g, Strehl %.4f" %
              (name, c["N"], int(FILES[name]["data"]["spup"].sum()), amplitude, sr))
        for k, v in FILES[name]["data"].items():
            out["%s_%s" % (name, k)] = v
        out["%s_tar_lambda" % name] = np.array(1.65)
        out["%s_otftel" % name], out["%s_otf2" % name], out["%s_psf" % name] = otftel, otf2, psf
    path = os.path.join(ROOT, "tests", "golden", "psf_rec_vii.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
