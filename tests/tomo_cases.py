"""Shared by tests/test_tomography.py and tests/test_gpu_tomography.py: the 10x10 system of lgs_cases.params with one more
p_targets entry at 25 arcsec (it declares the field: geometry.atmos_geometry sizes the screens for it), the two
constellations, and arbitrary points for the covariance."""
import numpy as np

from ao_marl_amd import geometry as G
from ao_marl_amd import system
from ao_marl_amd import tomography as T
from tests import lgs_cases as lc

FIELD = 25.0                        # arcsec
LAYERS_3 = (0., 4500., 14000.)
LAYERS_1 = (8000.,)
# A: 4 LGS at 90 km on a circle of 20 arcsec
STARS_A = T.ring(4, 20.0, 90e3)
# B: an on-axis NGS, an LGS at 90 km at (20, 0) and an LGS at 60 km at (-10, 15)
STARS_B = [(0., 0., np.inf), (20., 0., 90e3), (-10., 15., 60e3)]
_CACHE = {}


def params(alts):
    return T.with_field(lc.params(list(alts)), FIELD)


def system_of(alts):
    """(ParamSet, geometry.build_system result, SimArrays) with the declared field, built once per variant; read only"""
    key = tuple(alts)
    if key not in _CACHE:
        ps = params(alts)
        sysm = G.build_system(ps)
        _CACHE[key] = (ps, sysm, system.from_system(sysm, strehl_halfwin=8))
    return _CACHE[key]


def assert_footprints_inside(sysm, stars):
    """every star's footprint (the trace's coordinate at the pupil grid's corners) lies inside every screen"""
    off, dm1, delta = T.constellation_offsets(sysm, stars)
    n, c = int(sysm.geom.n), 0.5 * (int(sysm.geom.n) - 1)
    for k in range(off.shape[0]):
        for l in range(off.shape[1]):
            dim = int(sysm.atm.dim_screens[l])
            for ax in range(2):
                for x in (0., n - 1.):
                    f = (x + float(off[k, l, ax])) + float(dm1[k, l]) * (x - c)
                    assert 0. <= f <= dim - 1, (k, l, ax, f, dim)
    return off, dm1, delta


def layers_of(alts, r0=0.16, L0=None):
    """[(alt, r0_l, L0_l)] with equal fractions, as lgs_cases.params builds the atmosphere"""
    k = len(alts)
    return T.atmos_layers(alts, r0, np.full(k, 1.0 / k), np.full(k, 1e5) if L0 is None else L0)


def points(n, seed):
    """n arbitrary sub-aperture centres in metres inside a pupil of 2 m"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1., 1., n), rng.uniform(-1., 1., n)
