"""Shared by tests/test_mcao.py and tests/test_gpu_mcao.py: tomo_cases' system (lgs_cases.params with the 25 arcsec field
declared) in its pupdiam = 80 variant for the unit tests (sub-apertures of 8 pixels on N = 32) and at the derived
pupdiam = 160 for the closed loops, the two constellations, the mirrors and the footprint assertion."""
import numpy as np

from ao_marl_amd import field as F
from ao_marl_amd import geometry as G
from ao_marl_amd import mcao as M
from ao_marl_amd import system
from ao_marl_amd import tomography as T
from tests import lgs_cases as lc
from tests import tomo_cases as tc

FIELD = tc.FIELD                    # arcsec
STARS_A, STARS_B = tc.STARS_A, tc.STARS_B
LAYERS_1, LAYERS_3 = tc.LAYERS_1, tc.LAYERS_3
ALT_ONE = (8000.,)
ALT_TWO = (4500., 14000.)
SMALL = 80                          # pupdiam of the unit tests
LINE = F.line(20, 5)
_CACHE = {}


def params(alts, pupdiam=None):
    return T.with_field(lc.params(list(alts), pupdiam), FIELD)


def system_of(alts, pupdiam=None):
    """(ParamSet, geometry.build_system result, SimArrays) with the declared field, built once per variant; read only"""
    key = (tuple(alts), pupdiam)
    if key not in _CACHE:
        ps = params(alts, pupdiam)
        sysm = G.build_system(ps)
        _CACHE[key] = (ps, sysm, system.from_system(sysm, strehl_halfwin=8))
    return _CACHE[key]


def mirrors_of(sysm, alts):
    """altitude_mirror per altitude for the declared field, built once per (system, altitudes); read only"""
    key = ("mir", id(sysm), tuple(alts))
    if key not in _CACHE:
        _CACHE[key] = [M.altitude_mirror(sysm, h, FIELD) for h in alts]
    return _CACHE[key]


def assert_footprints_inside(sysm, mirrors, lookers, grid):
    """every looker's footprint (the coordinate at the grid's corners) lies inside every mirror's plane"""
    off, dm1 = M.mirror_offsets(sysm, mirrors, lookers, grid)
    nn = int(sysm.geom.n if grid == "wfs" else sysm.geom.pupdiam)
    c = 0.5 * (nn - 1)
    for k in range(off.shape[0]):
        for m, mir in enumerate(mirrors):
            for ax in range(2):
                for x in (0., nn - 1.):
                    f = (x + float(off[k, m, ax])) + float(dm1[k, m]) * (x - c)
                    assert 0. <= f <= mir.dim - 1, (k, m, ax, f, mir.dim)
    return off, dm1


def commands(mirrors, nenv, seed, scale=30.):
    """random commands [nenv][nact_total] (units of the mirror's command: 0.01 microns each at the peak)"""
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((nenv, sum(m.ntotact for m in mirrors)))).astype(np.float32)


def split(mirrors, v):
    o, out = 0, []
    for m in mirrors:
        out.append(v[..., o:o + m.ntotact])
        o += m.ntotact
    return out
