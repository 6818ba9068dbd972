"""Multi-conjugate AO on the device (csrc/aomarl_mcao.hip through ao_marl_amd/mcao.py): k_mcao_shape against
mirror_shape_model, aomarl_mcao_add against mirrors_add_model and its bits, a mirror at altitude 0 against the system's own
stack-array mirror, the science field through the mirrors, the refusals and the attachment's life cycle, the closed loop.

Tolerances (the convention of tests/test_gpu_field.py): the device computes in fp32 and is checked against the float64 model
within 4 x the error of the SAME model evaluated in float32 on the CPU, measured at run time; both numbers are printed.

Measured on an MI355X (device error, CPU float32 error): DESIGN.md, "Multi-conjugate AO"."""
import copy
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import field as F, geometry as G, libaomarl as la, mcao as M, tomography as T  # noqa: E402
from tests import mcao_cases as mcs  # noqa: E402

DEV = "cuda:0"
BIG = None                          # the derived pupdiam (160): the context is built for pdiam 16 / N 64 alone
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
FRACTIONAL = [(7.3, -11.9), (-10., 15.), (3.3, 4.4)]
RING17 = [(0., 0.)] + F.ring(16, 20.0)
FIELD_CASES = {"T1": [(0., 0.)], "T3": FRACTIONAL, "T16": F.ring(16, 20.0), "T17": RING17}
STARS_8 = mcs.STARS_A + [(0., 0., np.inf), (-10., 15., 60e3), (7.3, -11.9, np.inf), (3.3, 4.4, 90e3)]
DIRS_8 = FRACTIONAL + mcs.LINE


def _f64(t):
    return t.cpu().numpy().astype(np.float64)


def _check(what, dev, m64, m32):
    dev, m64, m32 = (np.asarray(a.cpu() if hasattr(a, "cpu") else a, dtype=np.float64) for a in (dev, m64, m32))
    eg, ec = np.abs(dev - m64).max(), np.abs(m32 - m64).max()
    print("    %-40s device %.3e  CPU float32 %.3e  (largest value %.4g)" % (what, eg, ec, np.abs(m64).max()))
    assert eg <= 4 * ec, what
    return eg, ec


@pytest.fixture(scope="module")
def state():
    """(SimArrays, system, HipSim of 3 environments of the three-layer system behind a reset, three moves and random
    mirror commands)"""
    from ao_marl_amd.sim import HipSim
    _, sysm, s = mcs.system_of(mcs.LAYERS_3, BIG)
    sim = HipSim(s, nenv=3, device=DEV, keep_phase=True)
    sim.reset([11, 12, 13])
    for _ in range(3):
        sim.move_atmos()
    rng = np.random.default_rng(2)
    sim.comp_dm_shape(torch.as_tensor(0.05 * rng.normal(size=(3, s.nactu)).astype(np.float32), device=DEV))
    return s, sysm, sim


def _native(sim, sysm, alts, seed=5):
    """(mirrors, NativeMcao with random commands shaped, the commands)"""
    mirrors = mcs.mirrors_of(sysm, alts)
    nm = M.NativeMcao(sim, mirrors)
    com = mcs.commands(mirrors, sim.nenv, seed)
    nm.apply(torch.as_tensor(com, device=DEV))
    return mirrors, nm, com


# ------------------------------------------------------------------------------------------------ 1. the shape
@pytest.mark.parametrize("alts", [mcs.ALT_ONE, mcs.ALT_TWO])
def test_shape_against_the_model(state, alts):
    """M = 1 and 2 (planes of different sides in one launch), random commands, one command on a corner actuator, zero"""
    s, sysm, sim = state
    mirrors, nm, com = _native(sim, sysm, alts)
    assert nm.M == len(alts) and len(set(nm.dims)) == len(alts)
    print("mirrors at %s m: dim %s, %s actuators" % (alts, nm.dims, [m.ntotact for m in mirrors]))
    for m, (mir, c) in enumerate(zip(mirrors, mcs.split(mirrors, com))):
        _check("mirror %d, random commands [um]" % m, nm.plane(m), M.mirror_shape_model(mir, c),
               M.mirror_shape_model(mir, c, np.float32))
    # a corner of the lattice: the first and the last actuator, the patch at the plane's edge
    corner = np.zeros_like(com)
    o = 0
    for mir in mirrors:
        corner[0, o], corner[1, o + mir.ntotact - 1], corner[2, o + mir.gw // 2] = 40., -25., 10.
        o += mir.ntotact
    nm.apply(torch.as_tensor(corner, device=DEV))
    for m, (mir, c) in enumerate(zip(mirrors, mcs.split(mirrors, corner))):
        m64 = M.mirror_shape_model(mir, c)
        assert np.abs(m64[0]).max() > 0.1 and np.abs(m64[1]).max() > 0.1
        _check("mirror %d, corner actuators [um]" % m, nm.plane(m), m64, M.mirror_shape_model(mir, c, np.float32))
        got = _f64(nm.plane(m))
        a = mir.ntotact - 1
        assert np.count_nonzero(got[1]) <= mir.ss**2 and got[1, mir.j1[a] + mir.ss // 2, mir.i1[a] + mir.ss // 2] != 0
    # a range of the environments leaves the others' planes; zero commands give an all-zero plane
    before = nm.planes.clone()
    nm.apply(torch.zeros(2, nm.nact_total, device=DEV), env_begin=1, env_count=2)
    assert torch.equal(nm.planes[0], before[0]) and float(nm.planes[1:].abs().max()) == 0
    nm.apply(torch.zeros(3, nm.nact_total, device=DEV))
    assert float(nm.planes.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 2. the add
def _whole_pixel(sysm, alt):
    """a direction whose shift on the mirror at `alt` is a whole number of pixels along x (10) and y (-7)"""
    per = G.ARCSEC2RAD * alt / float(sysm.atm.pupixsize)
    return (10. / per, -7. / per)


def _lookers(sysm, grid, K, alts):
    if grid == "wfs":
        return {1: [mcs.STARS_B[2]], 3: mcs.STARS_B, 4: mcs.STARS_A, 8: STARS_8}[K]
    return {1: [FRACTIONAL[0]], 3: FRACTIONAL, 4: [_whole_pixel(sysm, alts[0])] + FRACTIONAL, 8: DIRS_8}[K]


@pytest.mark.parametrize("alts", [mcs.ALT_ONE, mcs.ALT_TWO])
@pytest.mark.parametrize("grid", ["wfs", "pupil"])
def test_add_against_the_model(state, grid, alts):
    """K = 1, 3, 4, 8 on both grids, with and without the mask, onto planes that hold something; the shapes of the model
    are the device's planes"""
    s, sysm, sim = state
    mirrors, nm, _ = _native(sim, sysm, alts)
    shapes = [_f64(nm.plane(m)) for m in range(nm.M)]
    nn = s.n if grid == "wfs" else s.pupdiam
    pupil = np.asarray(s.mpupil if grid == "wfs" else s.spupil, dtype=np.float64).reshape(nn, nn)
    rng = np.random.default_rng(8)
    print("%s grid (%d pixels), mirrors at %s m:" % (grid, nn, alts))
    for K in (1, 3, 4, 8):
        off, dm1 = M.mirror_offsets(sysm, mirrors, _lookers(sysm, grid, K, alts), grid)
        base = (0.3 * rng.standard_normal((3, K, nn, nn))).astype(np.float32)
        m64 = M.mirrors_add_model(base.astype(np.float64), shapes, off, dm1)
        m32 = M.mirrors_add_model(base.copy(), [a.astype(np.float32) for a in shapes], off, dm1)
        assert np.abs(m64 - base).max() > 0.05
        got = nm.add(off, dm1, torch.as_tensor(base, device=DEV))
        _check("K = %d [um]" % K, got, m64, m32)
        masked = nm.add(off, dm1, torch.as_tensor(base, device=DEV), mask=True)
        _check("K = %d, masked" % K, masked, m64 * pupil, m32 * pupil.astype(np.float32))
        assert float(masked[:, :, pupil == 0].abs().max()) == 0
    if grid == "pupil":      # the whole-pixel direction: weights of zero, the floor cell's value exactly -- a shifted crop
        d = _whole_pixel(sysm, alts[0])
        off, dm1 = M.mirror_offsets(sysm, mirrors[:1], [d], "pupil")
        assert float(off[0, 0, 0]) == (mirrors[0].dim - nn) / 2 + 10 and float(off[0, 0, 1]) == (mirrors[0].dim - nn) / 2 - 7
        one = M.NativeMcao(sim, mirrors[:1])
        one.planes[:, 0, :mirrors[0].dim**2].copy_(nm.planes[:, 0, :mirrors[0].dim**2])
        got = one.add(off, dm1, torch.zeros(3, 1, nn, nn, device=DEV))
        x0, y0 = int(off[0, 0, 0]), int(off[0, 0, 1])
        assert torch.equal(got[:, 0], nm.plane(0)[:, y0:y0 + nn, x0:x0 + nn])


def test_add_bits(state):
    """plane (e, k) has the same bits alone (a K = 1 call), in any K and however the environments are split into calls"""
    s, sysm, sim = state
    mirrors, nm, _ = _native(sim, sysm, mcs.ALT_TWO)
    nn = s.n
    off, dm1 = M.mirror_offsets(sysm, mirrors, STARS_8, "wfs")
    base = torch.as_tensor((0.3 * np.random.default_rng(9).standard_normal((3, 8, nn, nn))).astype(np.float32), device=DEV)
    full = nm.add(off, dm1, base.clone())
    assert not torch.equal(full, base)
    for k in range(8):
        alone = nm.add(off[k:k + 1], dm1[k:k + 1], base[:, k:k + 1].clone())
        assert torch.equal(alone[:, 0], full[:, k]), k
    for sub in ([2, 5], [7, 0, 3], [1, 2, 3, 4, 6]):                     # KT = 2, 4, 8
        part = nm.add(off[sub], dm1[sub], base[:, sub].clone())
        assert torch.equal(part, full[:, sub]), sub
    split = base.clone()
    nm.add(off, dm1, split, env_begin=0, env_count=1)
    assert torch.equal(split[1:], base[1:])
    nm.add(off, dm1, split, env_begin=1, env_count=2)
    assert torch.equal(split, full)
    # with every command zero the planes stay what they were
    nm.reset()
    assert torch.equal(nm.add(off, dm1, base.clone()), base)


# ------------------------------------------------------------------------------------------------ 3. a mirror at altitude 0
def _ground(sysm, s):
    """(the mirror at altitude 0 on the ground pitch with the system's coupling, per system actuator its index there)"""
    pdm = sysm.params.p_dms[0]
    mir = M.altitude_mirror(sysm, 0., mcs.FIELD, coupling=float(pdm.coupling))
    d = sysm.dms[0]
    key = {(round(float(x), 3), round(float(y), 3)): a for a, (x, y) in
           enumerate(zip(mir.xpos - (mir.dim - 1) / 2., mir.ypos - (mir.dim - 1) / 2.))}
    idx = np.array([key[(round(float(x - sysm.geom.cent), 3), round(float(y - sysm.geom.cent), 3))] for x, y in zip(d.xpos, d.ypos)])
    return mir, idx


def test_mirror_at_altitude_zero_is_the_systems_own(state):
    """ground pitch, the system's stack-array commands: what it adds to every star's plane is what the system's own mirror
    adds (aomarl_tomo_trace with the mirrors only)"""
    s, sysm, sim = state
    mir, idx = _ground(sysm, s)
    npzt = int(sysm.dms[0].ntotact)
    rng = np.random.default_rng(4)
    volts = np.zeros((3, s.nactu), dtype=np.float32)
    volts[:, :npzt] = 30. * rng.standard_normal((3, npzt))
    mine = np.zeros((3, mir.ntotact), dtype=np.float32)
    mine[:, idx] = volts[:, :npzt]
    keep = sim.t["dm_shape"].clone()
    sim.comp_dm_shape(torch.as_tensor(volts, device=DEV))
    coff, cdm1, _ = T.constellation_offsets(sysm, mcs.STARS_B)
    own = T.NativeTomo(DEV).trace(sim, coff, cdm1, torch.zeros(3, 3, s.n, s.n, device=DEV), atm=False, dms=True)
    nm = M.NativeMcao(sim, [mir])
    nm.apply(torch.as_tensor(mine, device=DEV))
    off, dm1 = M.mirror_offsets(sysm, [mir], mcs.STARS_B, "wfs")
    assert float(np.abs(dm1).max()) == 0
    got = nm.add(off, dm1, torch.zeros(3, 3, s.n, s.n, device=DEV))
    zero = np.zeros((3, 3, s.n, s.n))
    m64 = M.mirrors_add_model(zero.copy(), [M.mirror_shape_model(mir, mine)], off, dm1)
    m32 = M.mirrors_add_model(zero.astype(np.float32), [M.mirror_shape_model(mir, mine, np.float32)], off, dm1)
    print("a mirror at altitude 0 against the system's own (%d of %d actuators):" % (npzt, mir.ntotact))
    _check("the attachment's mirror [um]", got, m64, m32)
    _check("the system's own mirror [um]", own, m64, m32)
    sim.t["dm_shape"].copy_(keep)


@pytest.mark.parametrize("delay", [1.0, 1.4, 2.0])
def test_delayed_voltage_is_the_simulators(delay):
    """the same command series through the simulator's delay line and through the attachment's: bit for bit"""
    from ao_marl_amd.sim import HipSim
    _, sysm, s0 = mcs.system_of(mcs.LAYERS_3, BIG)
    s = copy.copy(s0)
    s.delay = delay
    sim = HipSim(s, nenv=2, device=DEV)
    sim.reset([3, 4])
    mir, idx = _ground(sysm, s)
    npzt = int(sysm.dms[0].ntotact)
    nm = M.NativeMcao(sim, [mir])
    rng = np.random.default_rng(6)
    series = (20. * rng.standard_normal((6, 2, s.nactu))).astype(np.float32)
    want = M.delay_line_model(series[:, :, :npzt], delay)
    tidx = torch.as_tensor(idx, device=DEV)
    for t in range(6):
        sim.set_com(torch.as_tensor(series[t], device=DEV))
        sim.apply_control()
        nm.com.zero_()
        nm.com[:, tidx] = torch.as_tensor(series[t, :, :npzt], device=DEV)
        nm.apply()
        assert torch.equal(nm.voltage[:, tidx], sim.voltage[:, :npzt]), t
        assert t < 2 or float(nm.voltage.abs().max()) > 0
        # (the model rounds each product; the device may fuse: not the bits, a float32 rounding of the largest term)
        assert np.abs(nm.voltage[:, tidx].cpu().numpy() - want[t]).max() <= 2 * np.finfo(np.float32).eps * np.abs(series).max()
    # the planes are the delayed voltages' shapes
    sh = M.mirror_shape_model(mir, nm.voltage.cpu().numpy().astype(np.float64))
    _check("delay %g: planes of the delayed voltages" % delay, nm.plane(0), sh,
           M.mirror_shape_model(mir, nm.voltage.cpu().numpy(), np.float32))
    nm.reset(env_begin=1, env_count=1)
    assert float(nm.voltage[1].abs().max()) == 0 and float(nm.com[1].abs().max()) == 0 and float(nm.planes[1].abs().max()) == 0
    assert float(nm.voltage[0].abs().max()) > 0 and float(nm.planes[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4. the field
def _field_planes(sim, fld, shapes, dtype):
    scr = [sim.screen(l).cpu().numpy() for l in range(sim.s.nscreens)]
    sim.raytrace_target(atm=False, dms=True, reset=True)
    dm = sim.t["tar_phase"].cpu().numpy()
    out = []
    for e in range(sim.nenv):
        p = F.field_trace_model([a[e] for a in scr], fld.off, sim.s.pupdiam, dtype=dtype) + dm[e][None].astype(dtype)
        out.append(M.mirrors_add_model(p.astype(dtype), [a[e].astype(dtype) for a in shapes], *fld.mir_view))
    return np.stack(out)


@pytest.mark.parametrize("name", ["T1", "T3", "T16", "T17"])
def test_field_through_the_mirrors(state, name):
    """ScienceField(mirrors=...): the traced planes, the window and the record against FieldModel on the model's planes;
    with every command zero the field is the field without mirrors, bit for bit"""
    s, sysm, sim = state
    mirrors, nm, _ = _native(sim, sysm, mcs.ALT_TWO)
    shapes = [_f64(nm.plane(m)) for m in range(nm.M)]
    fld = F.ScienceField(sim, FIELD_CASES[name], sysm=sysm, mirrors=nm)
    plain = F.ScienceField(sim, FIELD_CASES[name], sysm=sysm)
    p64, p32 = _field_planes(sim, fld, shapes, np.float64), _field_planes(sim, fld, shapes, np.float32)
    print("%s through mirrors at %s m:" % (name, mcs.ALT_TWO))
    got = fld.trace()
    _check("traced planes [um]", got, p64, p32)
    assert float((got - plain.trace()).abs().max()) > 0.05
    assert torch.equal(fld.trace(dms=False), plain.trace(dms=False))
    m64, m32 = F.FieldModel(s), F.FieldModel(s, dtype=np.float32)
    st64, st32 = m64.new_state(3, fld.T), m32.new_state(3, fld.T)
    fld.observe()
    w64 = np.stack([m64.observe(p64[e], st64[0][e], st64[1][e]) for e in range(3)])
    w32 = np.stack([m32.observe(p32[e], st32[0][e], st32[1][e]) for e in range(3)])
    _check("window", fld.le_image(), w64, w32)
    rec = fld.record.cpu().numpy()
    for slot, what in ((0, "SE Strehl"), (2, "phase variance"), (6, "SE Strehl, fitted")):
        _check(what, rec[..., slot], st64[0][..., slot], st32[0][..., slot])
    # every command zero: the bits of a field that never saw a mirror
    nm.reset()
    fld.reset()
    fld.observe()
    plain.observe()
    fld.native.fit(), plain.native.fit()
    assert torch.equal(fld.native.record_view, plain.native.record_view) and torch.equal(fld.native.le_view, plain.native.le_view)
    assert torch.equal(fld.trace(), plain.trace())
    # detached, it is the plain field again whatever the mirrors hold
    nm.apply(torch.as_tensor(mcs.commands(mirrors, 3, 5), device=DEV))
    fld.native.detach_mirrors()
    assert torch.equal(fld.trace(), plain.trace())


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_reach_python_by_name(state):
    s, sysm, sim = state
    mirrors = mcs.mirrors_of(sysm, mcs.ALT_TWO)

    def changed(m, **kw):
        b = copy.copy(mirrors[m])
        for k, v in kw.items():
            setattr(b, k, v)
        return [b if i == m else x for i, x in enumerate(mirrors)]
    for bad, what in ((mirrors + mirrors[:1], "mcao_create: 3 mirrors: 1..2"), ([], "mcao_create: 0 mirrors: 1..2"),
                      (changed(1, alt=-1.), "mirror 1: alt = -1 m"), (changed(0, alt=np.nan), "mirror 0: alt"),
                      (changed(1, i1min=9), "mirror 1: the lattice leaves the plane"),
                      (changed(0, dim=100), "mirror 0: the lattice leaves the plane"),
                      (changed(0, grid=np.full_like(mirrors[0].grid, mirrors[0].ntotact)), "mirror 0: grid entry 0 = 285 outside -1..284"),
                      (changed(0, grid=np.full_like(mirrors[0].grid, -2)), "mirror 0: grid entry 0 = -2"),
                      (changed(1, pitch=5, gw=3, gh=3, ntotact=9, grid=np.arange(9, dtype=np.int32).reshape(3, 3)),
                       "larger than the shape kernel's LDS patch")):
        with pytest.raises(la.AomarlError, match=what):
            M.NativeMcao(sim, bad)
    # what three environments cannot reach through NativeMcao: create itself
    lib, out = la.load(), C.c_void_p()

    def create(nenv, d, outp=None):
        return lib.aomarl_mcao_create(sim.ctx, nenv, None if d is None else C.byref(d), C.byref(out) if outp is None else outp)
    d, keep_alive = M.mcao_desc(mirrors)
    nan_prof = keep_alive[3].copy()
    nan_prof[2] = np.nan
    for call, what in ((lambda: create(20000, d), "mcao_create: the planes of 20000 environments and 2 mirrors of 522 pixels exceed 2\^31 - 1"),
                       (lambda: create(0, d), "mcao_create: 0 environments: at least one"),
                       (lambda: create(-3, d), "environments: at least one"),
                       (lambda: create(3, None), "mcao_create: null desc"),
                       (lambda: lib.aomarl_mcao_create(sim.ctx, 3, C.byref(d), None), "mcao_create: null output pointer"),
                       (lambda: lib.aomarl_mcao_create(None, 3, C.byref(d), C.byref(out)), "mcao_create: null ctx")):
        assert call() == 1 and not out.value
        with pytest.raises(la.AomarlError, match=what):
            la.check(1)
    d.mirrors[1].grid = None
    assert create(3, d) == 1
    with pytest.raises(la.AomarlError, match="mirror 1: null grid / prof"):
        la.check(1)
    d, keep_alive = M.mcao_desc(mirrors)
    d.mirrors[0].prof = None
    assert create(3, d) == 1
    with pytest.raises(la.AomarlError, match="mirror 0: null grid / prof"):
        la.check(1)
    d.mirrors[0].prof = la.fptr(keep_alive[1])
    d.mirrors[1].prof = la.fptr(nan_prof)
    assert create(3, d) == 1 and not out.value
    with pytest.raises(la.AomarlError, match="mirror 1: prof\\[2\\] is not finite"):
        la.check(1)
    nm = M.NativeMcao(sim, mirrors)
    nn = s.n
    off, dm1 = M.mirror_offsets(sysm, mirrors, mcs.STARS_B, "wfs")
    planes = torch.full((3, 3, nn, nn), 7.0, device=DEV)
    keep = planes.clone()

    def add(o, d, p=planes, **kw):
        return lambda: nm.add(o, d, p, **kw)
    o_nan, o_far, d_bad = off.copy(), off.copy(), dm1.copy()
    o_nan[1, 0, 1], d_bad[2, 1] = np.inf, -1.0
    o_far[1, 1, 0] += 400.
    for call, what in ((add(np.tile(off, (3, 1, 1)), np.tile(dm1, (3, 1)), torch.zeros(3, 9, nn, nn, device=DEV)), "mcao_add: 9 directions: 1..8"),
                       (add(off[:2], dm1[:2]), "the view has 2 directions, the planes 3"),
                       (add(off, dm1, torch.zeros(3, 3, nn - 2, nn - 2, device=DEV)), "a grid of %d pixels" % (nn - 2)),
                       (add(o_nan, dm1), "off of direction 1, mirror 0 is not finite"),
                       (add(off, d_bad), "dm1 of direction 2, mirror 1 = -1"),
                       (add(o_far, dm1), "the footprint of direction 1 leaves mirror 1"),
                       (add(off, dm1, env_begin=2, env_count=2), "mcao_add: environments 2 .. \\+2 of 3"),
                       (lambda: nm.apply(env_begin=-1, env_count=1), "mcao_apply: environments"),
                       (lambda: nm.reset(env_begin=0, env_count=4), "mcao_reset: environments")):
        with pytest.raises(la.AomarlError, match=what):
            call()
    v = nm.view(off, dm1)
    lib = nm.lib
    assert lib.aomarl_mcao_add(nm.handle, sim.ctx, C.byref(v[0]), planes.data_ptr(), 3, nn, 0, 3, 4, nm._stream()) == 1
    with pytest.raises(la.AomarlError, match="mcao_add: unknown flags 4"):
        la.check(1)
    assert lib.aomarl_mcao_add(nm.handle, sim.ctx, C.byref(v[0]), None, 3, nn, 0, 3, 0, nm._stream()) == 1
    with pytest.raises(la.AomarlError, match="mcao_add: null planes"):
        la.check(1)
    assert lib.aomarl_mcao_add(nm.handle, sim.ctx, None, planes.data_ptr(), 3, nn, 0, 3, 0, nm._stream()) == 1
    with pytest.raises(la.AomarlError, match="mcao_add: null view"):
        la.check(1)
    empty = nm.view(off, dm1)
    empty[0].ndir = 0
    assert lib.aomarl_mcao_add(nm.handle, sim.ctx, C.byref(empty[0]), planes.data_ptr(), 3, nn, 0, 3, 0, nm._stream()) == 1
    with pytest.raises(la.AomarlError, match="mcao_add: 0 directions: 1..8"):
        la.check(1)
    for fn, what in ((lambda: lib.aomarl_mcao_apply(None, sim.ctx, 0, 3, None, nm._stream()), "mcao_apply: null argument"),
                     (lambda: lib.aomarl_mcao_reset(None, 0, 3, nm._stream()), "mcao_reset: null object"),
                     (lambda: lib.aomarl_mcao_com(None, None, None, None), "mcao_com: null object")):
        assert fn() == 1
        with pytest.raises(la.AomarlError, match=what):
            la.check(1)
    assert lib.aomarl_mcao_add(None, sim.ctx, C.byref(v[0]), planes.data_ptr(), 3, nn, 0, 3, 0, nm._stream()) == 1
    with pytest.raises(la.AomarlError, match="mcao_add: null argument"):
        la.check(1)
    with pytest.raises(ValueError, match="volts must be"):
        nm.apply(torch.zeros(3, 5, device=DEV))
    # the field: a view of another direction count, a cone
    fld = F.ScienceField(sim, FRACTIONAL, sysm=sysm)
    foff, fdm1 = M.mirror_offsets(sysm, mirrors, FRACTIONAL, "pupil")
    with pytest.raises(la.AomarlError, match="the view has 2 directions, the field 3"):
        fld.native.attach_mirrors(nm, foff[:2], fdm1[:2])
    with pytest.raises(la.AomarlError, match="a science direction is a natural star"):
        fld.native.attach_mirrors(nm, foff, fdm1 - 0.1)
    far = foff.copy()
    far[2, 0, 1] -= 300.
    with pytest.raises(la.AomarlError, match="field_attach_mirrors: the footprint of direction 2 leaves mirror 0"):
        fld.native.attach_mirrors(nm, far, fdm1)
    with pytest.raises(ValueError, match="leaves mirror"):
        M.mirror_offsets(sysm, mirrors, [(60., 0.)], "pupil")
    # a prefetched reset in flight
    sim.prefetch_reset_begin([21, 22, 23])
    try:
        with pytest.raises(la.AomarlError, match="mcao_add: a prefetched reset is in flight"):
            nm.add(off, dm1, planes)
        with pytest.raises(la.AomarlError, match="mcao_apply: a prefetched reset is in flight"):
            nm.apply()
    finally:
        sim.reset([21, 22, 23])
    torch.cuda.synchronize()
    assert torch.equal(planes, keep) and float(nm.planes.abs().max()) == 0


def test_a_pipelined_frame_in_flight_is_refused_by_the_library():
    from ao_marl_amd.env import VecAoEnv
    env = VecAoEnv(mcs.params(mcs.LAYERS_1, BIG), 3, RL, n_agents_modal=1, frame_pipeline=True)
    sup = env.supervisor
    mirrors = mcs.mirrors_of(sup.sysm, mcs.ALT_ONE)
    nm = M.NativeMcao(sup.sim, mirrors)
    env.reset()
    zero = torch.zeros(3, env.action_dim, device=DEV)
    for _ in range(3):
        env.step(zero)
    assert sup.sim.frame_pipeline_state()[0], "no pipelined frame in flight: this test needs one"
    off, dm1 = M.mirror_offsets(sup.sysm, mirrors, mcs.STARS_A, "wfs")
    with pytest.raises(la.AomarlError, match="mcao_add: the frame pipeline is on"):
        nm.add(off, dm1, torch.zeros(3, 4, sup.s.n, sup.s.n, device=DEV))
    with pytest.raises(la.AomarlError, match="mcao_apply: the frame pipeline is on"):
        nm.apply()
    with pytest.raises(RuntimeError, match="MultiConjugate.start: the frame pipeline is on|LgsSensor.start: the frame pipeline is on"):
        mc = M.MultiConjugate(sup, mcs.STARS_A, mirrors=mirrors, noise=-1, reconstructor="mean")
        mc.cmat = mc.cmat_tomo = mc.cmat_ground = np.zeros((1, 1))
        mc.start()


# ------------------------------------------------------------------------------------------------ 6. the attachment
@pytest.fixture(scope="module")
def loop_pair():
    """two supervisors of the one-layer system on the same seeds, 3 environments; the first gets the attachments"""
    from ao_marl_amd.env import VecRlSupervisor
    return [VecRlSupervisor(mcs.params(mcs.LAYERS_1, BIG), RL, 3) for _ in range(2)]


def _frames(sup, nframes):
    sup.reset()
    sup.next_part_one()
    for _ in range(nframes):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()
    torch.cuda.synchronize()
    return [t.clone() for t in (sup.get_slopes(), sup.get_command(), sup.get_strehl())]


def _on_axis_against_the_loops_own_path(sup, mc):
    """Under the attached ls loop with the altitude mirrors in use: direction (0, 0) of ScienceField(mirrors=mc) against
    the loop's own science path (frame(): raytrace_target + add + target_psf_buffer; next_part_two: comp_strehl;
    get_strehl()), three frames on the same states -- the field observes between next_part_one and next_part_two, the state
    the frame just imaged.  The allowance is test_gpu_field.py's for this comparison: 4 x the float32 model's error of the
    same figure, measured here against the float64 model.  Without the mirrors the same state reads another Strehl.
    The supervisor is built with prefetch_atmos=False: with the screens a frame ahead there is no moment at which an
    observer sees the state the frame imaged."""
    sim = sup.sim
    assert not sup.prefetch_atmos
    assert float(mc.alt_voltage.abs().max()) > 0
    on = mc.field([(0., 0.)])
    m64, m32 = F.FieldModel(sup.s), F.FieldModel(sup.s, dtype=np.float32)
    st64, st32 = m64.new_state(3, 1), m32.new_state(3, 1)
    sup.next_part_two(None, linear_control=True)                   # (the pending frame of _frames is committed)
    sim.reset_strehl()
    for _ in range(3):
        sup.next_part_one()
        on.observe()
        keep = sim.t["tar_phase"].clone()
        shapes = [_f64(p) for p in mc.alt_shapes()]
        p64, p32 = _field_planes(sim, on, shapes, np.float64), _field_planes(sim, on, shapes, np.float32)
        sim.t["tar_phase"].copy_(keep)
        for e in range(3):
            m64.observe(p64[e], st64[0][e], st64[1][e])
            m32.observe(p32[e], st32[0][e], st32[1][e])
        bare = F.ScienceField(sim, [(0., 0.)], sysm=sup.sysm)      # (on the simulator: it does not know the attachment)
        bare.observe()
        sup.next_part_two(None, linear_control=True)
    own, own_fit = sup.get_strehl(do_fit=False).cpu().numpy(), sup.get_strehl().cpu().numpy()
    got, got_fit = on.strehl(do_fit=False).cpu().numpy()[:, 0], on.strehl().cpu().numpy()[:, 0]
    assert float(on.record[..., 4].min()) == 3 and float(sim.t["strehl"][:, 4].min()) == 3
    ec = np.abs(np.asarray(st32[0]) - st64[0])
    print("direction (0, 0) through the mirrors against the loop's own get_strehl():")
    for col, what in enumerate(("SE Strehl", "LE Strehl", "phase variance", "mean variance")):
        for tag, a, b, slot in (("", got, own, (0, 1, 2, 3)[col]), (", fitted", got_fit, own_fit, (6, 7, 2, 3)[col])):
            tol = 4 * (ec[..., slot].max() / (3.0 if col == 3 else 1.0))
            d = np.abs(a[:, col] - b[:, col]).max()
            print("    %-28s field - loop %.3e  4 x CPU float32 %.3e  (value %.4f)" % (what + tag, d, tol, b[:, col].mean()))
            assert d <= tol, what + tag
    without = bare.strehl(do_fit=False).cpu().numpy()[:, 0, 0]
    print("    SE Strehl of the last state without the add: %s against %s" % (without, own[:, 0]))
    assert np.all(np.abs(without - own[:, 0]) > 0.01)


def test_life_cycle(loop_pair):
    sup, never = loop_pair
    mc = M.MultiConjugate(sup, mcs.STARS_A, mirrors=[(8000.,)], field_radius=mcs.FIELD, noise=-1)
    assert M.MultiConjugate.slot == "lgs" and isinstance(mc, T.LaserTomography)
    with pytest.raises(RuntimeError, match="calibrate\\(\\) first"):
        mc.start()
    with pytest.raises(ValueError, match="3 mirrors: 1..2"):
        M.MultiConjugate(sup, mcs.STARS_A, mirrors=[(1e3,), (2e3,), (3e3,)])
    with pytest.raises(ValueError, match="reconstructor 'tomo'"):
        M.MultiConjugate(sup, mcs.STARS_A, reconstructor="tomo")
    with pytest.raises(ValueError, match="leaves mirror"):
        M.MultiConjugate(sup, mcs.STARS_A, mirrors=[(8000.,)], field_radius=0.)
    with pytest.raises(NotImplementedError, match="polc"):
        M.MultiConjugate(sup, mcs.STARS_A, polc=True)
    with pytest.raises(NotImplementedError, match="set_atmosphere"):
        mc.set_atmosphere(r0=0.1)
    cg, ca = mc.calibrate()
    print("calibration: D %s, %d of %d singular values cut at maxcond %g, stars' responses differ by %.3g" % (
        mc.D_ls.shape, mc.ncut, mc.svals.size, mc.maxcond, mc.star_match))
    assert cg.shape == (sup.s.nactu, 4 * sup.s.nslope) and ca.shape == (mc.nact_total, 4 * sup.s.nslope)
    assert mc.ncut == int(np.sum(mc.svals < mc.svals[0] / mc.maxcond)) and 0 < mc.ncut < mc.svals.size
    assert np.abs(ca).max() > 0 and float(mc.alt_com.abs().max()) == 0
    # with the altitude commands zero the traced planes are the parent's, bit for bit
    parent = T.LaserTomography(sup, mcs.STARS_A, noise=-1, reconstructor="mean", polc=False)
    sup.reset()
    sup.sim.move_atmos()
    mc.trace()
    parent.trace()
    assert torch.equal(mc.planes, parent.planes) and float(mc.planes.abs().max()) > 0
    # a field without the mirrors refuses while the attachment is on
    plain = F.ScienceField(sup, mcs.LINE)
    mc.start()
    try:
        assert sup.lgs is mc and sup.sensing is mc
        with pytest.raises(RuntimeError, match="ScienceField.observe: a MultiConjugate is attached"):
            plain.observe()
        fld = mc.field(mcs.LINE)
        got = _frames(sup, 6)
        assert float(mc.alt_com.abs().max()) > 0 and float(mc.alt_voltage.abs().max()) > 0
        assert all(float(p.abs().max()) > 0 for p in mc.alt_shapes())
        assert sup.get_slopes() is mc.est and tuple(mc.est.shape) == (3, sup.s.nslope)
        assert torch.allclose(mc.est, mc.star_slopes.view(3, 4, -1).mean(1), atol=1e-6)
        fld.observe()
        assert float(fld.record[..., 4].min()) == 1
        F.ScienceField(sup, [(0., 0.)], mirrors=mc.mc).observe()       # the device object that owns the planes will do
        # reset() zeroes the altitude state
        sup.reset()
        torch.cuda.synchronize()
        assert float(mc.alt_com.abs().max()) == 0 and float(mc.alt_voltage.abs().max()) == 0
        assert all(float(p.abs().max()) == 0 for p in mc.alt_shapes())
    finally:
        mc.stop()
    assert sup.lgs is None and sup.sensing is None
    plain.observe()
    # stop() restores the loop bit for bit
    after, base = _frames(sup, 3), _frames(never, 3)
    assert all(torch.equal(a, b) for a, b in zip(after, base))
    assert not torch.equal(got[1], base[1])


def test_on_axis_field_against_the_loops_own_strehl():
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(mcs.params(mcs.LAYERS_1, BIG), RL, 3, prefetch_atmos=False)
    mc = M.MultiConjugate(sup, mcs.STARS_A, mirrors=[(8000.,)], field_radius=mcs.FIELD, noise=-1)
    mc.calibrate()
    mc.start()
    try:
        _frames(sup, 6)
        _on_axis_against_the_loops_own_path(sup, mc)
    finally:
        mc.stop()


def test_mean_with_the_mirrors_at_rest_is_the_parents_loop(loop_pair):
    """reconstructor "mean": the commands of LaserTomography("mean", polc=False) bit for bit; the Strehl through the
    buffer (raytrace_target + add of zeros + target_psf_buffer against target_psf): the same phase to the bit through two
    kernels that order the DFT's sums differently.  A Strehl is the square of a float32 sum of N = pupdiam^2 pi / 4 = 2e4
    terms over a constant: the two orders differ by a few sqrt(N) eps = 140 x 6e-8 = 8e-6 of a value below 1: 1e-5."""
    sup, _ = loop_pair
    parent = T.LaserTomography(sup, mcs.STARS_A, noise=-1, reconstructor="mean", polc=False)
    parent.calibrate()
    parent.start()
    want = _frames(sup, 5)
    parent.stop()
    mc = M.MultiConjugate(sup, mcs.STARS_A, mirrors=[(8000.,)], field_radius=mcs.FIELD, noise=-1, reconstructor="mean")
    mc.calibrate()
    mc.start()
    got = _frames(sup, 5)
    mc.stop()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert float(mc.alt_com.abs().max()) == 0
    d = float((got[2] - want[2]).abs().max())
    print("mean, mirrors at rest: Strehl through the buffer against the parent's path: %.3e" % d)
    assert d <= 1e-5


# ------------------------------------------------------------------------------------------------ 7. the closed loop
def test_closed_loop_corrects_the_field():
    """10x10, one layer at 8000 m, 4 environments x 300 frames on the same seeds, fitted long-exposure Strehl along
    line(20, 5): MCAO ls with one mirror at 8000 m against the NGS integrator and LaserTomography("tomo", polc=True),
    computed here.  Strict inequalities, no margin."""
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(mcs.params(mcs.LAYERS_1), RL, 4)
    nframes = 300
    ngs, own_ngs = F.strehl_against_angle(sup, mcs.LINE, nframes)
    lt = T.LaserTomography(sup, mcs.STARS_A, reconstructor="tomo", polc=True)
    lt.calibrate()
    lt.start()
    ltao, own_lt = F.strehl_against_angle(sup, mcs.LINE, nframes)
    lt.stop()
    mc = M.MultiConjugate(sup, mcs.STARS_A, mirrors=[(8000.,)], field_radius=mcs.FIELD)
    mc.calibrate()
    mc.start()
    mcao, own_mc = F.strehl_against_angle(sup, mcs.LINE, nframes, mirrors=mc)
    mc.stop()
    print("field angle [arcsec]        " + "".join("%8.1f" % d[0] for d in mcs.LINE) + "   loop's own")
    for name, row, own in (("NGS integrator", ngs, own_ngs), ("LTAO tomo, polc", ltao, own_lt),
                           ("MCAO ls (%d of %d cut)" % (mc.ncut, mc.svals.size), mcao, own_mc)):
        print("%-28s" % name + "".join("%8.4f" % v for v in row) + "   %8.4f" % own)
    assert mcao[3] > ngs[3] and mcao[3] > ltao[3]
    assert mcao[4] > ngs[4] and mcao[4] > ltao[4]
    assert mcao[4] / mcao[0] > ngs[4] / ngs[0]
