"""A scalar restatement of the science field's trace, written independently of ao_marl_amd/field.py for
tests/test_field.py: one pixel at a time, the four bilinear taps written out.  Plain Python floats (float64)."""
import math

import numpy as np


def tap(screen, dim, ix, iy):
    return float(screen[iy][ix])


def trace_pixel(screens, off_d, x, y):
    """the phase at pupil pixel (x, y) for one direction: layers in order; zero outside a screen; the last line clamped"""
    total = 0.0
    for l, scr in enumerate(screens):
        dim = len(scr)
        fx = float(x) + float(off_d[l][0])
        fy = float(y) + float(off_d[l][1])
        ix, iy = int(math.floor(fx)), int(math.floor(fy))
        wx, wy = fx - ix, fy - iy
        if ix < 0 or iy < 0 or ix >= dim or iy >= dim:
            total = total + 0.0
            continue
        ix1 = ix + 1 if ix + 1 < dim else ix
        iy1 = iy + 1 if iy + 1 < dim else iy
        v00, v01 = tap(scr, dim, ix, iy), tap(scr, dim, ix1, iy)
        v10, v11 = tap(scr, dim, ix, iy1), tap(scr, dim, ix1, iy1)
        top = (1.0 - wx) * v00 + wx * v01
        bot = (1.0 - wx) * v10 + wx * v11
        total = total + ((1.0 - wy) * top + wy * bot)
    return total


def trace_planes(screens, off, pupdiam):
    """[T][pupdiam][pupdiam] float64"""
    out = np.zeros((len(off), pupdiam, pupdiam))
    for d in range(len(off)):
        for y in range(pupdiam):
            for x in range(pupdiam):
                out[d, y, x] = trace_pixel(screens, off[d], x, y)
    return out
