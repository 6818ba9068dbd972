"""The parameter sets the GPU tests of the mirror mis-registration run (tests/test_gpu_registration.py), pinned here so
that tests/test_registration.py can prove their conditioning without a GPU: on the 10x10 system's two grids and two
mirrors no sample comes within 1e-3 pixel of a plane's border (u or v = 0 or dim: the only places where the bilinear
rule jumps), and every case has samples that leave the plane, samples in the clamped last row and last column, and
negative coordinates.

One qualification.  A whole-pixel shift that walks off the plane puts a sample ON u = 0 and on u = dim: it cannot be
otherwise.  Those samples are harmless for the reason the margin exists at all -- the margin keeps fp32 round-off of a
coordinate from changing the side of a jump, and the coordinates of the whole-pixel cases have no round-off: fp32 and
float64 give the same number, bit for bit.  `conditioning` therefore measures the gap over the samples whose fp32
position differs from the float64 one, and reports separately whether every sample of a case is exact; the test
asserts `exact` for the integer and the quarter-turn case and the gap for all three."""
import numpy as np

from ao_marl_amd import registration as R

NAME = "production_sh_10x10_2m"
NENV = 4
# the 10x10 system as geometry.build_system gives it (checked against it by test_registration.py)
PIXSIZE = 0.0125                                  # metres per pupil pixel
PITCH = 16.0                                      # pixels between actuators of the stack-array mirror
DIMS = (258, 272)                                 # stack array, tip-tilt
GRIDS = {"wfs": (164, ((47.0, 47.0), (54.0, 54.0))), "tar": (160, ((49.0, 49.0), (56.0, 56.0)))}
MARGIN = 1e-3


def _rows(A, t):
    return R.rows_of(np.asarray(A, dtype=np.float64), np.asarray(t, dtype=np.float64))


def integer_case():
    """whole-pixel shifts, another one per environment and mirror: rows [ndm][nenv][6]"""
    eye = np.eye(2)
    m0 = [_rows(eye, t) for t in ((-60, 55), (52, -49), (47, 47), (-3, 11))]
    m1 = [_rows(eye, t) for t in ((62, -58), (-57, 54), (54, 54), (5, -2))]
    return np.stack([np.stack(m0), np.stack(m1)])


def quarter_case():
    """A = [[0, -1], [1, 0]] and its three powers, with whole-pixel shifts"""
    q = np.array([[0.0, -1.0], [1.0, 0.0]])
    p = [q, q @ q, q @ q @ q, q]
    m0 = [_rows(p[e], t) for e, t in enumerate(((0, 0), (-55, 50), (50, -52), (47, 47)))]
    m1 = [_rows(p[e], t) for e, t in enumerate(((0, 0), (57, -60), (-59, 56), (54, 54)))]
    return np.stack([np.stack(m0), np.stack(m1)])


# dx, dy in pixels (the tests multiply by PIXSIZE: the surface takes metres), theta in radians, G
FRACTIONAL = (
    # mirror 0 (stack array), one line per environment
    ((0.37 * PITCH, -0.21 * PITCH, np.deg2rad(1.0), 1.0),
     (-3.3, 7.9, np.deg2rad(-0.35), 1.013),
     (8.25, 0.6, 0.004, 0.987),
     (6.25, -4.5, np.deg2rad(3.0), 0.6)),
    # mirror 1 (tip-tilt)
    ((0.0, 0.0, np.deg2rad(2.0), 1.0),
     (1.7, -2.2, np.deg2rad(-1.2), 1.02),
     (-6.4, 3.1, 0.0, 0.97),
     (-4.15, 6.65, np.deg2rad(-2.5), 0.58)),
)


def fractional_case():
    out = []
    for mirror in FRACTIONAL:
        p = np.array(mirror, dtype=np.float64)
        A, t = R.registration_affine(p[:, 0] * PIXSIZE, p[:, 1] * PIXSIZE, p[:, 2], p[:, 3], PIXSIZE)
        out.append(R.rows_of(A, t))
    return np.stack(out)


CASES = {"integer": integer_case, "quarter": quarter_case, "fractional": fractional_case}


def conditioning(rows):
    """dict of the facts the conditioning test asserts, over every environment, mirror and grid of a case (float64
    sample positions of the fp32 rows)"""
    gap, leaves, last_row, last_col, negative, exact = np.inf, False, False, False, False, True
    for nn, offsets in GRIDS.values():
        for k, dim in enumerate(DIMS):
            for e in range(rows.shape[1]):
                u, v = R.sample_positions(nn, offsets[k], rows[k, e], np.float64)
                u32, v32 = R.sample_positions(nn, offsets[k], rows[k, e], np.float32)
                for w, w32 in ((u, u32), (v, v32)):
                    rounded = w32.astype(np.float64) != w
                    exact &= not bool(rounded.any())
                    if rounded.any():
                        gap = min(gap, np.abs(w[rounded]).min(), np.abs(w[rounded] - dim).min())
                inside = (u >= 0) & (v >= 0) & (u < dim) & (v < dim)
                leaves |= bool((~inside).any())
                negative |= bool((u < 0).any() or (v < 0).any())
                last_col |= bool((inside & (np.floor(u) == dim - 1)).any())
                last_row |= bool((inside & (np.floor(v) == dim - 1)).any())
    return dict(gap=gap, exact=exact, leaves=leaves, last_row=last_row, last_col=last_col, negative=negative)
