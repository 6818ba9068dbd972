"""The slopes-only frame kernel takes the three moments of a sub-aperture from FOUR matrix products
(csrc/aomarl_spot_dev.h: spot_qf_moments): both Toeplitz kernels factor through one real basis,

    M = H' H'^T,      S = H' L H'^T,      L = 2 x 2 blocks [[0, t_k], [-t_k, 0]],

so that with P = H'^T E H' (E H' and then H'^T . for the real and the imaginary part)  sum I = |P|^2  and the first
moments pair neighbouring columns / rows of P_r and P_i with t_k.  Checked here on the CPU:
(a) the identity for arbitrary real Er, Ei in float64 with a basis computed by numpy alone,
(b) the table the library itself builds (csrc/aomarl_qf4_host.h, compiled into a stand-alone program: nothing is
    loaded into this process): H' H'^T = M, H' L H'^T = S and the sign / factor convention of its lane layout,
(c) the float32 centroids with the library's basis against the definition and against the six-product form."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import qf_cog_check as qf  # noqa: E402


def _moments6(M, S, Er, Ei):
    """sum I, sum (X - 7.5) I, sum (Y - 7.5) I of the six-product form (the reference of this file)."""
    cx, cy, s0 = qf.cog_quadratic_form_six(M, S, None, None, np.float64, field=(Er, Ei))
    return s0, (cx - 7.5) * s0, (cy - 7.5) * s0


def _scale(M, S, Er, Ei):
    A, Sa, E2 = np.abs(M), np.abs(S), np.abs(Er) + np.abs(Ei)
    return max((A * (E2 @ A @ E2.T)).sum(), (Sa * (E2 @ A @ E2.T)).sum(), (A * (E2 @ Sa @ E2.T)).sum())


def _fields(rng, n):
    for trial in range(n):
        Er, Ei = rng.normal(size=(2, 16, 16)) * rng.uniform(0.1, 30.0)
        if trial % 3:
            mask = rng.random((16, 16)) > 0.3
            Er, Ei = Er * mask, Ei * mask
        if trial % 5 == 0:
            Ei = Ei * 0.0                                         # a purely real field: both first moments vanish
        yield trial, Er, Ei


def test_four_products_hold_all_three_moments_for_any_real_field():
    """(a) Nothing in the identity uses |E| = 1 or the mask.  Bound: the moments are sums of 16^4 products accumulated
    in float64 and the factorisation of M, S by LAPACK is good to a few eps of their norm; 1e-10 of the sum of the
    magnitudes (the scale of tests/test_qf_six_products.py) is orders above both."""
    M, S = qf.kernels()
    H, t = qf.four_product_basis()
    assert np.abs(H @ H.T - M).max() < 1e-12 * np.abs(M).max()
    L = np.zeros((16, 16))
    L[np.arange(0, 16, 2), np.arange(1, 16, 2)], L[np.arange(1, 16, 2), np.arange(0, 16, 2)] = t, -t
    assert np.abs(H @ L @ H.T - S).max() < 1e-12 * np.abs(S).max()
    for trial, Er, Ei in _fields(np.random.default_rng(11), 60):
        cx, cy, s0 = qf.cog_four_products(H, t, None, None, np.float64, field=(Er, Ei))
        got = (s0, (cx - 7.5) * s0, (cy - 7.5) * s0)
        scale = _scale(M, S, Er, Ei)
        for x, y in zip(got, _moments6(M, S, Er, Ei)):
            assert abs(x - y) <= 1e-10 * scale, (trial, x, y, scale)


# ------------------------------------------------------------------------------------------ the library's own table
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """What tools/qf4_table.cpp prints: (err_m, err_s, t [8], H' [16, 16] in double, the float [64, 8] lane table)."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++ or $CXX)"
    exe = str(tmp_path_factory.mktemp("qf4") / "qf4_table")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ao_marl_amd", "csrc"),
                           os.path.join(ROOT, "tools", "qf4_table.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    rows = {k: [np.array(l.split()[1:], dtype=np.float64) for l in out if l.split()[0] == k] for k in ("err", "t", "H", "lane")}
    tab = np.stack(rows["lane"]).astype(np.float32)
    assert tab.shape == (64, 8) and np.stack(rows["H"]).shape == (16, 16)
    return rows["err"][0][0], rows["err"][0][1], rows["t"][0], np.stack(rows["H"]), tab


def _lane_column(c):
    return (c & ~3) | ((c & 1) << 1) | ((c >> 1) & 1)


def _undo_layout(tab):
    """H' [x][a] and t [8] out of the lane table (lane = 16 q + c): [0..3] = H'[4q + s][lane_column(c)],
    [4], [5] = -2 t_{2q}, -2 t_{2q+1}, [6] = +-t_{lane_column(c) >> 1} (+ on the even column of the pair), [7] = 0."""
    tab = tab.astype(np.float64)
    H, t = np.empty((16, 16)), np.empty(8)
    for lane in range(64):
        q, a = lane >> 4, _lane_column(lane & 15)
        H[4 * q:4 * q + 4, a] = tab[lane, 0:4]
        assert tab[lane, 4] == tab[16 * q, 4] and tab[lane, 5] == tab[16 * q, 5] and tab[lane, 7] == 0.0
        t[2 * q], t[2 * q + 1] = -0.5 * tab[lane, 4], -0.5 * tab[lane, 5]
    for lane in range(64):
        a = _lane_column(lane & 15)
        assert tab[lane, 6] == (-1.0 if a & 1 else 1.0) * np.float32(t[a >> 1]), lane
    return H, t


def test_library_table_factors_both_kernels(table):
    """(b) The program's double basis meets M and S to 1e-12 of their norm (the check the library makes before it
    uploads), and its float table does to float32 rounding of a double table: every constant is off by at most
    2^-24 of itself, so an element of H' H'^T by 2 . 2^-24 sum |H'| |H'| and one of H' L H'^T by 3 . 2^-24
    sum |H'| t |H'| (first order; 1 % on top for the second).  Through the identities, not element by element:
    the basis is not unique."""
    err_m, err_s, t64, H64, tab = table
    assert err_m <= 1e-12 and err_s <= 1e-12, (err_m, err_s)
    assert (t64 > 0).all()
    M, S = qf.kernels()
    H, t = _undo_layout(tab)
    assert np.array_equal(H.astype(np.float32), H64.astype(np.float32)) and np.array_equal(t.astype(np.float32), t64.astype(np.float32))
    L = np.zeros((16, 16))
    L[np.arange(0, 16, 2), np.arange(1, 16, 2)], L[np.arange(1, 16, 2), np.arange(0, 16, 2)] = t, -t
    La = np.abs(L)
    u = 2.0 ** -24
    dm, ds = np.abs(H @ H.T - M), np.abs(H @ L @ H.T - S)
    bm, bs = 1.01 * 2 * u * (np.abs(H) @ np.abs(H).T), 1.01 * 3 * u * (np.abs(H) @ La @ np.abs(H).T)
    print("float table: |H'H'^T - M| max %.3g (bound %.3g), |H'LH'^T - S| max %.3g (bound %.3g)" % (dm.max(), bm.max(), ds.max(), bs.max()))
    assert (dm <= bm + 1e-12).all() and (ds <= bs + 1e-12).all()
    assert np.abs(H64 @ H64.T - M).max() <= 1e-12 * np.linalg.norm(M)


def _lane_moments(tab, Er, Ei):
    """The kernel's arithmetic on the lane table, in float64: rows 0, 1, 2 of the moments as the tile loop stores
    them (sum I, -sum (Y - 7.5) I, sum (X - 7.5) I / 2)."""
    tab = tab.astype(np.float64)
    h = np.empty((16, 16))                                        # h[x][c]: the operand of lane column c
    for lane in range(64):
        h[4 * (lane >> 4):4 * (lane >> 4) + 4, lane & 15] = tab[lane, 0:4]
    Pr, Pi = h.T @ Er @ h, h.T @ Ei @ h                           # [i = 4q + r][c]
    s0 = ty = tx = 0.0
    for lane in range(64):
        q, c = lane >> 4, lane & 15
        r_, i_ = Pr[4 * q:4 * q + 4, c], Pi[4 * q:4 * q + 4, c]
        s0 += (r_ * r_).sum() + (i_ * i_).sum()
        ty += tab[lane, 4] * (i_[0] * r_[2] - i_[2] * r_[0]) + tab[lane, 5] * (i_[1] * r_[3] - i_[3] * r_[1])
        tx += tab[lane, 6] * (i_ * Pr[4 * q:4 * q + 4, c ^ 2]).sum()
    return s0, ty, tx


def test_library_table_sign_and_factor_convention(table):
    """(b) The lane arithmetic of spot_qf_moments on the library's table gives row 0 = sum I, row 1 = -sum (Y - 7.5) I
    whole, row 2 = sum (X - 7.5) I / 2 -- what qf_slopes and the once-per-stripe slope step expect -- against the
    six-product form.  Bound: seven float32 constants enter every term (four h and a t, each 2^-24 off), first order
    5 . 2^-24 of the sum of the magnitudes; 1e-6 of that scale."""
    M, S = qf.kernels()
    tab = table[4]
    for trial, Er, Ei in _fields(np.random.default_rng(12), 12):
        s0, mx, my = _moments6(M, S, Er, Ei)
        got = _lane_moments(tab, Er, Ei)
        scale = _scale(M, S, Er, Ei)
        for x, y in zip(got, (s0, -my, 0.5 * mx)):
            assert abs(x - y) <= 1e-6 * scale, (trial, got, (s0, -my, 0.5 * mx), scale)
    # a pure x tilt moves the x centroid only, towards larger X for a phase that grows with x -- and likewise in y
    for ax, rev in ((1, 1.5), (0, -2.25)):
        ph = np.arange(16) * rev / 16.0
        ph = ph[None, :] + np.zeros((16, 1)) if ax == 1 else ph[:, None] + np.zeros((1, 16))
        E = np.exp(2j * np.pi * ph)
        s0, ty, tx = _lane_moments(tab, E.real, E.imag)
        cx, cy = 7.5 + 2 * tx / s0, 7.5 - ty / s0
        dx, dy = (cx - 7.5, cy - 7.5)
        moved, still = (dx, dy) if ax == 1 else (dy, dx)
        assert abs(still) < 1e-5 and np.sign(moved) == np.sign(rev) and abs(moved) > 0.3 * abs(rev), (ax, rev, cx, cy)


def _wfs(name):
    from ao_marl_amd import params, geometry
    return geometry.build_system(params.builtin(name)).wfss[0]


def test_float32_centroids_against_definition_and_six_products(table):
    """(c) Products in float32 with the library's basis, on the 200 cases of qf_cog_check.main() plus 100 with tilts
    of up to +-6 revolutions per sub-aperture and pistons of up to +-300: the centroid against the FFT definition
    below the tool's own 2e-5 pixel, and not worse than 1.5 x the six-product form's error on the same inputs (the
    margin covers the different rounding order)."""
    w = _wfs("production_sh_40x40_8m_3layers")
    assert (w.Nfft, w.pdiam, w.npix, w.nrebin) == (64, 16, 16, 2)
    M, S = qf.kernels()
    _, _, t, H, _ = table
    rng = np.random.default_rng(1)                                # (the generator and the draws of qf_cog_check.main)
    cases = []
    for trial in range(200):
        amp = (rng.random((16, 16)) > (0.0 if trial % 2 else 0.2)).astype(float)
        tilt = np.add.outer(np.arange(16) * rng.normal() * 0.08, np.arange(16) * rng.normal() * 0.08)
        cases.append((rng.normal(size=(16, 16)) * rng.uniform(0, 0.5) + tilt, amp))
    for trial in range(100):
        amp = (rng.random((16, 16)) > (0.0 if trial % 2 else 0.25)).astype(float)
        tx, ty = rng.uniform(-6.0, 6.0, size=2)
        tilt = np.add.outer(np.arange(16) * ty / 16.0, np.arange(16) * tx / 16.0)
        cases.append((rng.normal(size=(16, 16)) * rng.uniform(0, 0.3) + tilt + rng.uniform(-300.0, 300.0), amp))
    worst4 = worst6 = worst4_64 = 0.0
    for ph, amp in cases:
        a = qf.cog_definition(w, ph, amp)
        b4 = qf.cog_four_products(H, t, ph, amp, np.float64)
        c4 = qf.cog_four_products(H, t, ph, amp, np.float32)
        c6 = qf.cog_quadratic_form_six(M, S, ph, amp, np.float32)
        worst4_64 = max(worst4_64, abs(a[0] - b4[0]), abs(a[1] - b4[1]))
        worst4 = max(worst4, abs(a[0] - c4[0]), abs(a[1] - c4[1]))
        worst6 = max(worst6, abs(a[0] - c6[0]), abs(a[1] - c6[1]))
        assert abs(a[2] - c4[2]) < 2e-6 * a[2]
    print("worst centroid error, pixels: four products float64 %.3g, float32 %.3g; six products float32 %.3g" % (worst4_64, worst4, worst6))
    assert worst4_64 < 1e-6
    assert worst4 < 2e-5
    assert worst4 <= 1.5 * worst6
