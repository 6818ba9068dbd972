"""Independent statements the registration tests compare ao_marl_amd.registration.trace_model with: the plain ray
trace of the existing kernel (k_raytrace: every mirror at its fixed offset), written pixel by pixel, and the exact
pictures of a plane under an integer shift and a quarter turn, written with slices."""
import numpy as np


def plain_trace(nn, planes, offsets, dtype=np.float64, start=None):
    """k_raytrace's mirror part, one pixel at a time: fx = x + ox, floor, zero outside, clamped neighbour, shortcut."""
    out = np.zeros((nn, nn), dtype=dtype) if start is None else np.array(start, dtype=dtype)
    dt = np.dtype(dtype).type
    for plane, (ox, oy) in zip(planes, offsets):
        p = np.asarray(plane).astype(dtype)
        dim = p.shape[0]
        for y in range(nn):
            fy = dt(y) + dt(oy)
            iy = int(np.floor(fy))
            for x in range(nn):
                fx = dt(x) + dt(ox)
                ix = int(np.floor(fx))
                if ix < 0 or iy < 0 or ix >= dim or iy >= dim:
                    continue
                wx, wy = fx - dt(ix), fy - dt(iy)
                ix1, iy1 = min(ix + 1, dim - 1), min(iy + 1, dim - 1)
                if wx == 0 and wy == 0:
                    out[y, x] += p[iy, ix]
                else:
                    out[y, x] += (1 - wy) * ((1 - wx) * p[iy, ix] + wx * p[iy, ix1]) + \
                        wy * ((1 - wx) * p[iy1, ix] + wx * p[iy1, ix1])
    return out


def shifted_picture(plane, nn, offset, shift):
    """out[y, x] = plane[y + oy + sy, x + ox + sx] where that pixel exists, 0 elsewhere (integers throughout)"""
    dim = plane.shape[0]
    ox, oy, sx, sy = int(offset[0]), int(offset[1]), int(shift[0]), int(shift[1])
    out = np.zeros((nn, nn), dtype=plane.dtype)
    for y in range(nn):
        py = y + oy + sy
        if py < 0 or py >= dim:
            continue
        x0, x1 = max(0, -(ox + sx)), min(nn, dim - (ox + sx))
        if x1 > x0:
            out[y, x0:x1] = plane[py, x0 + ox + sx:x1 + ox + sx]
    return out


def quarter_turn_picture(plane, nn, o):
    """the picture through A = [[0, -1], [1, 0]], t = 0 of a plane at the integer offset (o, o) that covers the window:
    u = (nn - 1) + o - y, v = o + x, i.e. the window turned by a quarter"""
    w = plane[o:o + nn, o:o + nn]
    assert w.shape == (nn, nn)
    return np.rot90(w, 1).copy()
