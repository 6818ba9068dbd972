"""Float64 references for the AO frame at large phase (tests/test_phase_range_reference.py on the CPU,
tests/test_gpu_phase_range.py on the GPU).

A field Delta = P K, with P the common period of the sensor and science wavelengths and K any integer field, leaves
exp(2 pi i phase / lambda) unchanged at every pixel for both wavelengths: it moves no slope, no spot, no PSF and no
Strehl ratio, only the phase variance -- while it drives |phase| (and |phase - phase at the pupil centre|) as far past
the +-256 revolutions of v_sin_f32 / v_cos_f32 as one wants."""
import math
import os
import sys
import types
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import qf_cog_check  # noqa: E402


def common_period(s):
    """Smallest P > 0 that is a whole number of both wavelengths (um): 16.5 = 33 x 0.5 = 10 x 1.65 for the shipped
    configurations.  Exact in fp32, and so is every P K with |K| <= 2^24 / (2 P)."""
    fw = Fraction(float(s.wfs_lambda)).limit_denominator(1000)
    ft = Fraction(float(s.tar_lambda)).limit_denominator(1000)
    num = fw.numerator * ft.numerator // math.gcd(fw.numerator, ft.numerator)
    P = Fraction(num, math.gcd(fw.denominator, ft.denominator))
    assert (P / fw).denominator == 1 and (P / ft).denominator == 1
    assert float(np.float32(float(P))) == float(P)
    return float(P)


def pupil_centre_on_layer(s, layer):
    """Screen pixel (row, column) that the kernels' pivot -- the phase at the centre of the pupil grid -- reads from
    `layer` (ring origin 0, as after set_screen)."""
    half = s.pupdiam // 2
    ox, oy = s.tar_atm_off[layer]
    return half + int(oy), half + int(ox)


def piston_field(dim, k):
    """K = k everywhere (a whole-layer piston)."""
    return np.full((dim, dim), int(k), dtype=np.int64)


def block_field(dim, rng, kmax=40, block=5, centre=None, clear=0):
    """Random integers in [-kmax, kmax] per block x block pixels (5 x 5 blocks: steps inside every 16-pixel
    sub-aperture), the extremes +-kmax both present, K = 0 within `clear` pixels (Chebyshev) of `centre`."""
    nb = -(-dim // block)
    K = rng.integers(-kmax, kmax + 1, size=(nb, nb))
    K = np.kron(K, np.ones((block, block), dtype=np.int64))[:dim, :dim]
    K[0, 0], K[-1, -1] = kmax, -kmax
    if centre is not None:
        r, c = centre
        K[max(r - clear, 0):r + clear + 1, max(c - clear, 0):c + clear + 1] = 0
    return K


def ramp_field(dim, slope=0.37, kmax=40):
    """A steep ramp rounded to integers: K(y, x) = round(slope (x + 0.6 y)), clipped to [-kmax, kmax]."""
    y, x = np.mgrid[0:dim, 0:dim]
    return np.clip(np.rint(slope * (x + 0.6 * y - 0.8 * dim)), -kmax, kmax).astype(np.int64)


def offset_field(P, K):
    """Delta = P K as float32 (exact: P and every P K below 2^24 ulps are fp32 numbers)."""
    d = (float(P) * np.asarray(K, dtype=np.float64))
    out = d.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), d)
    return out


# ------------------------------------------------------------------------------------------------------------ slopes
def wfs_view(s):
    """What qf_cog_check.cog_definition reads of a sensor."""
    return types.SimpleNamespace(Nfft=int(s.nfft), pdiam=int(s.pdiam), npix=int(s.npix),
                                 halfxy=np.asarray(s.halfxy, np.float64).reshape(s.pdiam, s.pdiam),
                                 binmap=np.asarray(s.binmap).reshape(s.nrebin * s.nrebin, s.npix * s.npix))


def subap_sample(s, nmax=None, seed=0):
    """Sub-aperture indices: all of them, or every edge one (fewer than 4 valid neighbours) plus about nmax others."""
    if nmax is None or s.nvalid <= nmax:
        return np.arange(s.nvalid)
    vx, vy = np.asarray(s.validsubsx), np.asarray(s.validsubsy)
    pos = set(zip(vx.tolist(), vy.tolist()))
    st = int(s.pdiam)
    edge = [i for i in range(s.nvalid)
            if sum((vx[i] + dx, vy[i] + dy) in pos for dx, dy in ((st, 0), (-st, 0), (0, st), (0, -st))) < 4]
    rest = np.setdiff1d(np.arange(s.nvalid), edge)
    pick = np.random.default_rng(seed).choice(rest, size=min(nmax, rest.size), replace=False)
    return np.union1d(np.asarray(edge, dtype=np.int64), pick)


def slopes64(s, wfs_phase, subaps=None):
    """Noise-free slopes (arcsec, x block then y block, NaN where not computed) of a sensor phase [n, n] (um, as the
    raytrace leaves it, or float64): the float64 centre of gravity of the spot (qf_cog_check.cog_definition) of
    exp(2 pi i mod(phase / lambda, 1)), the phase converted to float64 first."""
    w = wfs_view(s)
    ph = np.asarray(wfs_phase).astype(np.float64).ravel()
    amp = np.asarray(s.mpupil, np.float64).ravel()
    pm = np.asarray(s.phasemap).reshape(s.pdiam * s.pdiam, s.nvalid)
    out = np.full(2 * s.nvalid, np.nan)
    for i in (range(s.nvalid) if subaps is None else subaps):
        p = pm[:, i]
        rev = np.mod(ph[p] / float(s.wfs_lambda), 1.0).reshape(s.pdiam, s.pdiam)
        cx, cy, _ = qf_cog_check.cog_definition(w, rev, amp[p].reshape(s.pdiam, s.pdiam))
        out[i] = (cx - s.cog_offset) * s.cog_scale
        out[s.nvalid + i] = (cy - s.cog_offset) * s.cog_scale
    return out


# ----------------------------------------------------------------------------------------------------------- science
def psf_window64(s, tar_phase):
    """|FFT|^2 of the pupil field on the npsf grid, at the 2 hw x 2 hw frequencies around 0 the Strehl ratio reads
    (the oracle's aoref_psf window: row j, column i <-> (ky, kx) = (j - hw, i - hw)), in float64 as a direct DFT."""
    n, N, hw = s.pupdiam, s.npsf, s.strehl_halfwin
    ph = np.asarray(tar_phase).astype(np.float64)
    E = np.asarray(s.spupil, np.float64) * np.exp(2j * np.pi * np.mod(ph / float(s.tar_lambda), 1.0))
    k = np.arange(-hw, hw)
    W = np.exp(-2j * np.pi * np.outer(k, np.arange(n)) / N)          # [2 hw, n]
    F = W @ E @ W.T                                                   # [ky, kx]
    return np.abs(F) ** 2


def strehl64(s, tar_phase):
    """Short-exposure Strehl ratio of the window peak: max |F|^2 / (sum of the pupil)^2."""
    return float(psf_window64(s, tar_phase).max()) / float(np.sum(s.spupil, dtype=np.float64)) ** 2


def phase_var64(s, tar_phase):
    """Variance of the phase over the pupil (um^2), the oracle's aoref_phase_var in float64 throughout."""
    ph = np.asarray(tar_phase, np.float32).astype(np.float64)[np.asarray(s.spupil) > 0]
    return float(np.mean((ph - ph.mean()) ** 2))


# ------------------------------------------------------------------------------------ the oracle's own rounding
def oracle_arg_error(s, maxabs, lam):
    """Worst error (radians) of the oracle's fp32 argument  fl(fl(phase) * fl(2 pi / lambda))  at |phase| <= maxabs
    (um), against 2 pi phase / lambda of the exact phase: rounding of phase (1/2 ulp), of the constant (1/2 ulp
    relative) and of the product (1/2 ulp)."""
    sc = float(np.float32(2.0 * np.pi / lam))
    big = maxabs * sc
    ulp = lambda v: float(np.spacing(np.float32(v)))                  # noqa: E731
    return 0.5 * ulp(maxabs) * sc + abs(sc - 2.0 * np.pi / lam) * maxabs + 0.5 * ulp(big)
