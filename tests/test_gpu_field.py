"""The science field on the device (csrc/aomarl_field.hip through ao_marl_amd/field.py): aomarl_field_trace against the
float64 model and against the simulator's own target trace, aomarl_field_observe against FieldModel, direction (0, 0)
against the simulator's own PSF chain, the bits (environment splits, other directions, launches of a field with more than
16 directions, reset), that nothing else moves, the device-side refusals and the closed loop.

Tolerances (the convention of tests/test_gpu_lgs.py and tests/test_gpu_tomography.py): the device computes in fp32 and is
checked against the float64 model within 4 x the error of the SAME model evaluated in float32 on the CPU, measured at run
time; both numbers are printed."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import field as F, libaomarl as la, system  # noqa: E402
from tests import tomo_cases as tc  # noqa: E402

DEV = "cuda:0"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
FRACTIONAL = [(7.3, -11.9), (-10., 15.), (3.3, 4.4)]
RING17 = [(0., 0.)] + F.ring(16, 20.0)
CASES = {"T1": [(0., 0.)], "T3": FRACTIONAL, "T16": F.ring(16, 20.0), "T17": RING17}


def _state(hw):
    """(SimArrays, system, HipSim of 3 environments behind a reset, three moves and random mirror commands)"""
    from ao_marl_amd.sim import HipSim
    _, sysm, s8 = tc.system_of(tc.LAYERS_3)
    s = s8 if hw == 8 else system.from_system(sysm, strehl_halfwin=hw)
    sim = HipSim(s, nenv=3, device=DEV, keep_phase=True)
    sim.reset([11, 12, 13])
    for _ in range(3):
        sim.move_atmos()
    rng = np.random.default_rng(2)
    sim.comp_dm_shape(torch.as_tensor(0.05 * rng.normal(size=(3, s.nactu)).astype(np.float32), device=DEV))
    return s, sysm, sim


@pytest.fixture(scope="module")
def traced():
    return _state(8)


@pytest.fixture(scope="module")
def traced16():
    return _state(16)


def _screens(sim):
    return [sim.screen(l).cpu().numpy() for l in range(sim.s.nscreens)]


def _mirrors(sim):
    """the mirrors' plane on the target's grid [nenv][pd][pd], as the simulator's own trace gives it"""
    sim.raytrace_target(atm=False, dms=True, reset=True)
    return sim.t["tar_phase"].cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. the trace
@pytest.mark.parametrize("name", ["T3", "T17"])
def test_trace_against_the_model(traced, name):
    s, sysm, sim = traced
    fld = F.ScienceField(sim, CASES[name], sysm=sysm)
    scr = _screens(sim)
    got = fld.trace(atm=True, dms=False).cpu().numpy().astype(np.float64)
    eg = ec = 0.0
    for e in range(3):
        layers = [a[e] for a in scr]
        m64 = F.field_trace_model(layers, fld.off, s.pupdiam)
        m32 = F.field_trace_model(layers, fld.off, s.pupdiam, dtype=np.float32).astype(np.float64)
        eg, ec = max(eg, np.abs(got[e] - m64).max()), max(ec, np.abs(m32 - m64).max())
    print("%s: atmosphere [um]: device %.3e  CPU float32 %.3e  (largest phase %.3f)" % (name, eg, ec, np.abs(got).max()))
    assert eg <= 4 * ec
    # off-axis planes are not the on-axis one (a trace that ignored the offsets would give it back)
    on_axis = F.ScienceField(sim, [(0., 0.)], sysm=sysm).trace(atm=True, dms=False).cpu().numpy()
    for d in range(fld.T):
        if tuple(CASES[name][d]) != (0., 0.):
            assert np.abs(got[:, d] - on_axis[:, 0]).max() > 1e-3, d
    # the mirrors on top; alone they are the simulator's own mirror plane in every direction, to the bit
    dm_only = _mirrors(sim)
    assert np.abs(dm_only).max() > 0
    only = fld.trace(atm=False, dms=True)
    assert all(torch.equal(only[:, d], sim.t["tar_phase"]) for d in range(fld.T))
    both = fld.trace().cpu().numpy().astype(np.float64)
    assert np.abs(both - (got + dm_only[:, None])).max() <= 4 * ec + 1e-6 * np.abs(got).max()
    # however the environments are split into calls, the same bits; rows outside the range stay
    part = fld.trace(env_begin=1, env_count=2)
    assert torch.equal(part[1:], torch.as_tensor(both, dtype=torch.float32, device=DEV)[1:]) and float(part[0].abs().max()) == 0


def test_on_axis_trace_is_the_simulators_to_the_bit(traced):
    """direction (0, 0): whole-pixel offsets, bilinear weights of zero -- sim.raytrace_target's tar_phase bit for bit,
    alone and as direction 0 of the 17"""
    s, sysm, sim = traced
    one = F.ScienceField(sim, [(0., 0.)], sysm=sysm).trace()
    big = F.ScienceField(sim, RING17, sysm=sysm).trace()
    sim.raytrace_target(atm=True, dms=True, reset=True)
    assert torch.equal(one[:, 0], sim.t["tar_phase"]) and torch.equal(big[:, 0], sim.t["tar_phase"])
    assert float(one.abs().max()) > 0
    sim.raytrace_target(atm=True, dms=False, reset=True)
    assert torch.equal(F.ScienceField(sim, [(0., 0.)], sysm=sysm).trace(dms=False)[:, 0], sim.t["tar_phase"])


# ------------------------------------------------------------------------------------------------ 2. observe
def _models(s, Lambda=None):
    return F.FieldModel(s, Lambda), F.FieldModel(s, Lambda, dtype=np.float32)


def _observe_both(sim, fld, m64, m32, st64, st32):
    """one observe on the device and on both models (their planes: the model's trace of the device's screens in that
    precision + the simulator's mirror plane); returns the models' windows"""
    scr, dm = _screens(sim), _mirrors(sim)
    fld.observe()
    w64, w32 = [], []
    for e in range(sim.nenv):
        layers = [a[e] for a in scr]
        p64 = F.field_trace_model(layers, fld.off, sim.s.pupdiam) + dm[e][None]
        p32 = (F.field_trace_model(layers, fld.off, sim.s.pupdiam, dtype=np.float32) + dm[e][None].astype(np.float32)).astype(np.float32)
        w64.append(m64.observe(p64, st64[0][e], st64[1][e]))
        w32.append(m32.observe(p32, st32[0][e], st32[1][e]))
    return np.stack(w64), np.stack(w32)


def _check(what, dev, w64, w32):
    dev, w64, w32 = (np.asarray(a, dtype=np.float64) for a in (dev, w64, w32))
    eg, ec = np.abs(dev - w64).max(), np.abs(w32 - w64).max()
    print("    %-28s device %.3e  CPU float32 %.3e  (largest value %.4g)" % (what, eg, ec, np.abs(w64).max()))
    assert eg <= 4 * ec, what


@pytest.mark.parametrize("hw", [8, 16])
@pytest.mark.parametrize("name", ["T1", "T3", "T16", "T17"])
def test_observe_against_the_model(traced, traced16, name, hw):
    """the window, slots 0, 2 and 6 behind one observe; behind three (the atmosphere moved in between) slots 1, 3, 4, 7 and
    le_image().  T = 17 runs as two launches."""
    s, sysm, sim = traced if hw == 8 else traced16
    fld = F.ScienceField(sim, CASES[name], sysm=sysm)
    m64, m32 = _models(s)
    st64, st32 = m64.new_state(3, fld.T), m32.new_state(3, fld.T)
    print("%s, strehl_halfwin %d:" % (name, hw))
    w64, w32 = _observe_both(sim, fld, m64, m32, st64, st32)
    W = 2 * hw
    pend = fld.le_image().cpu().numpy()                       # one frame: the window itself
    assert pend.shape == (3, fld.T, W, W)
    _check("window", pend, w64, w32)
    rec = fld.record.cpu().numpy()
    for slot, what in ((0, "SE Strehl"), (2, "phase variance"), (6, "SE Strehl, fitted")):
        _check(what, rec[..., slot], st64[0][..., slot], st32[0][..., slot])
    assert np.all(rec[..., 4] == 1) and np.array_equal(rec[..., 5], st64[0][..., 5])
    for _ in range(2):
        sim.move_atmos()
        _observe_both(sim, fld, m64, m32, st64, st32)
    rec = fld.record.cpu().numpy()
    for slot, what in ((1, "LE Strehl"), (3, "sum of the variances"), (7, "LE Strehl, fitted")):
        _check(what, rec[..., slot], st64[0][..., slot], st32[0][..., slot])
    assert np.all(rec[..., 4] == 3)
    _check("long-exposure window", fld.le_image().cpu().numpy(), st64[1] / 3.0, st32[1] / 3.0)
    st = fld.strehl().cpu().numpy()
    assert st.shape == (3, fld.T, 4) and np.array_equal(st[..., 1], rec[..., 7]) and np.allclose(st[..., 3], rec[..., 3] / 3.0)
    assert np.array_equal(fld.strehl(do_fit=False).cpu().numpy()[..., 0], rec[..., 0])


def test_on_axis_against_the_simulators_own_chain(traced):
    """direction (0, 0) against sim.target_psf + comp_strehl + strehl_fit on the same state: SE and LE Strehl, plain and
    fitted, the variance, the window.  Another order of the DFT's sums: the same tolerance, not the bits."""
    s, sysm, sim = traced
    fld = F.ScienceField(sim, [(0., 0.)], sysm=sysm)
    m64, m32 = _models(s)
    st64, st32 = m64.new_state(3, 1), m32.new_state(3, 1)
    sim.reset_strehl()
    for k in range(2):
        if k:
            sim.move_atmos()
        sim.target_psf()
        sim.comp_strehl()
        _observe_both(sim, fld, m64, m32, st64, st32)
    own, own_fit = sim.strehl.cpu().numpy(), sim.strehl_fit.cpu().numpy()
    got, got_fit = fld.strehl(do_fit=False).cpu().numpy()[:, 0], fld.strehl().cpu().numpy()[:, 0]
    print("direction (0, 0) against the simulator's own chain:")
    for col, what in enumerate(("SE Strehl", "LE Strehl", "phase variance", "mean variance")):
        ec = np.abs(np.asarray(st32[0]) - st64[0])
        for tag, a, b, slot in (("", got, own, (0, 1, 2, 3)[col]), (", fitted", got_fit, own_fit, (6, 7, 2, 3)[col])):
            tol = 4 * (ec[..., slot].max() / (2.0 if col == 3 else 1.0))
            print("    %-28s field - simulator %.3e  4 x CPU float32 %.3e" % (what + tag, np.abs(a[:, col] - b[:, col]).max(), tol))
            assert np.abs(a[:, col] - b[:, col]).max() <= tol, what + tag
    le_own = sim.t["le_img"].reshape(3, 16, 16).cpu().numpy() / 2.0
    _check("long-exposure window", le_own, st64[1][:, 0] / 2.0, st32[1][:, 0] / 2.0)
    assert np.abs(fld.le_image().cpu().numpy()[:, 0] - le_own).max() <= 4 * np.abs(st32[1] - st64[1]).max() / 2.0


# ------------------------------------------------------------------------------------------------ 3. the bits
def _bits(fld):
    fld.native.fit()
    torch.cuda.synchronize()
    return fld.native.record_view.clone(), fld.native.le_view.clone()


def test_bits(traced):
    s, sysm, sim = traced
    whole = F.ScienceField(sim, RING17, sysm=sysm)
    whole.observe()
    whole.observe()
    rec, le = _bits(whole)
    assert float(rec[..., 4].min()) == 2 and float(le.min()) >= 0 and float(rec[..., 0].min()) > 0
    # the environments split [0, 1) + [1, 3)
    split = F.ScienceField(sim, RING17, sysm=sysm)
    for _ in range(2):
        split.observe(env_begin=0, env_count=1)
        split.observe(env_begin=1, env_count=2)
    r2, l2 = _bits(split)
    assert torch.equal(r2, rec) and torch.equal(l2, le)
    # direction d of the 17 (d = 16 falls into the second launch) in a field of its own, and among three
    for d in (0, 5, 15, 16):
        own = F.ScienceField(sim, [RING17[d]], sysm=sysm)
        own.observe()
        own.observe()
        r1, l1 = _bits(own)
        assert torch.equal(r1[:, 0], rec[:, d]) and torch.equal(l1[:, 0], le[:, d]), d
    three = F.ScienceField(sim, [RING17[16], RING17[3], RING17[0]], sysm=sysm)
    three.observe()
    three.observe()
    r3, l3 = _bits(three)
    for k, d in enumerate((16, 3, 0)):
        assert torch.equal(r3[:, k], rec[:, d]) and torch.equal(l3[:, k], le[:, d]), d
    # reset(): observing twice behind it is observing twice on a fresh object; a partial reset leaves the rest
    split.observe()
    split.reset(env_begin=1, env_count=2)
    r4, l4 = _bits(split)
    assert float(r4[1:].abs().max()) == 0 and float(l4[1:].abs().max()) == 0 and float(r4[0, :, 4].min()) == 3
    split.reset()
    split.observe()
    split.observe()
    r5, l5 = _bits(split)
    assert torch.equal(r5, rec) and torch.equal(l5, le)


# ------------------------------------------------------------------------------------------------ 4. nothing else moves
def test_observe_leaves_the_state_alone(traced):
    s, sysm, sim = traced
    sim.raytrace_target()
    sim.raytrace_wfs()
    sim.target_psf()                                                   # a pending PSF window in the workspace
    sim.comp_strehl()
    torch.cuda.synchronize()
    names = ("tar_phase", "strehl", "le_img", "wfs_phase", "work", "slopes", "com", "voltage", "dm_shape", "screens", "origin")
    before = {k: sim.t[k].clone() for k in names}
    fld = F.ScienceField(sim, RING17, sysm=sysm)
    fld.observe()
    fld.trace()
    fld.record
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(sim.t[k], before[k]), k
    sim.comp_strehl()                                                  # the pending slot is still the simulator's
    assert float(sim.t["strehl"][:, 4].min()) == float(before["strehl"][:, 4].min()) + 1


@pytest.fixture(scope="module")
def loop():
    from ao_marl_amd.env import VecRlSupervisor
    return VecRlSupervisor(tc.params(tc.LAYERS_1), RL, 4)


def _frames(sup, nframes, fld=None):
    sup.reset()
    if fld is not None:
        fld.reset()
    for _ in range(nframes):
        sup.next_part_one()
        sup.next_part_two(None, linear_control=True)
        if fld is not None:
            fld.observe()
    return [t.clone() for t in (sup.get_slopes(), sup.get_command(), sup.get_err(), sup.get_voltages(), sup.get_strehl())]


def test_the_loop_does_not_notice_an_observer(loop):
    sup = loop
    fld = F.ScienceField(sup, F.line(20, 5))
    plain = _frames(sup, 5)
    watched = _frames(sup, 5, fld)
    assert all(torch.equal(a, b) for a, b in zip(plain, watched))
    assert float(fld.record[..., 4].min()) == 5 and sup.sensing is None and sup.control_law is None
    assert all(torch.equal(a, b) for a, b in zip(plain, _frames(sup, 5)))


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_device_side_refusals():
    """a prefetched reset in flight, a bad range, an unknown flag: the error by name, nothing launched (the record and the
    long-exposure sum stay as they were); create's refusals come from the host half"""
    s, sysm, sim = _state(8)
    fld = F.ScienceField(sim, FRACTIONAL, sysm=sysm)
    fld.observe()
    rec, le = _bits(fld)
    nat, lib = fld.native, fld.native.lib

    def call(fn, b, n, flags, *more):
        args = (nat.handle, sim.ctx, C.byref(sim.st)) + more + (b, n, flags, nat._stream())
        return fn(*args)
    planes = torch.full((3, 3, s.pupdiam, s.pupdiam), 7.0, dtype=torch.float32, device=DEV)
    keep = planes.clone()
    for b, n, flags, what in ((2, 2, 3, "field_observe: environments 2 .. \\+2 of 3"), (-1, 1, 3, "field_observe: environments"),
                              (0, 0, 3, "field_observe: environments"), (0, 3, 4, "field_observe: unknown flags 4"),
                              (0, 3, 19, "field_observe: unknown flags 19")):
        assert call(lib.aomarl_field_observe, b, n, flags) == 1
        with pytest.raises(la.AomarlError, match=what):
            la.check(1)
    assert call(lib.aomarl_field_trace, 0, 3, 16 | 7, planes.data_ptr()) == 1
    with pytest.raises(la.AomarlError, match="field_trace: unknown flags 23"):
        la.check(1)
    assert lib.aomarl_field_trace(nat.handle, sim.ctx, C.byref(sim.st), None, 0, 3, 7, nat._stream()) == 1
    with pytest.raises(la.AomarlError, match="field_trace: null planes"):
        la.check(1)
    assert lib.aomarl_field_reset(nat.handle, 1, 3, nat._stream()) == 1
    with pytest.raises(ValueError, match="planes must be"):
        nat.trace(planes[:, :2])
    # a state of another size
    from ao_marl_amd.sim import HipSim
    other = HipSim(s, nenv=2, device=DEV)
    assert lib.aomarl_field_observe(nat.handle, other.ctx, C.byref(other.st), 0, 2, 3, nat._stream()) == 1
    with pytest.raises(la.AomarlError, match="the field has 3 environments, the state 2"):
        la.check(1)
    # a prefetched reset in flight: the object's own refusal first, the library's behind it
    sim.prefetch_reset_begin([21, 22, 23])
    try:
        with pytest.raises(RuntimeError, match="ScienceField.observe: a prefetched reset is in flight"):
            fld.observe()
        with pytest.raises(RuntimeError, match="ScienceField.trace: a prefetched reset is in flight"):
            fld.trace()
        with pytest.raises(la.AomarlError, match="field_observe: a prefetched reset is in flight"):
            nat.observe()
        with pytest.raises(la.AomarlError, match="field_trace: a prefetched reset is in flight"):
            nat.trace(planes)
    finally:
        sim.reset([21, 22, 23])                                        # adopts the prefetch
    # the frame pipeline with a frame in flight: the object's own refusal (the library's is aomarl_tomo_trace's text)
    sim._twin, sim.frame_pipeline_state = object(), lambda: (True, False, 1, 0)
    try:
        with pytest.raises(RuntimeError, match="ScienceField.observe: a pipelined frame is in flight"):
            fld.observe()
    finally:
        sim._twin = None
        del sim.frame_pipeline_state
    r2, l2 = _bits(fld)
    assert torch.equal(r2, rec) and torch.equal(l2, le) and torch.equal(planes, keep)
    # create: the host half's refusals reach the caller by name
    with pytest.raises(la.AomarlError, match="field_create: offsets for 2 layers, the context has 3"):
        F.NativeField(sim, fld.off[:, :2], 1.65)
    bad = fld.off.copy()
    bad[1, 2, 0] = np.nan
    with pytest.raises(la.AomarlError, match="off of direction 1, layer 2 is not finite"):
        F.NativeField(sim, bad, 1.65)
    bad = fld.off.copy()
    bad[2, 1, 1] += 300.
    with pytest.raises(la.AomarlError, match="footprint of direction 2 leaves screen 1"):
        F.NativeField(sim, bad, 1.65)
    with pytest.raises(la.AomarlError, match="at least one direction"):
        F.NativeField(sim, fld.off[:0], 1.65)
    fld.observe()                                                      # and the object still works
    assert float(fld.record[..., 4].min()) == 2


def test_a_pipelined_frame_in_flight_is_refused_by_the_library():
    from ao_marl_amd.env import VecAoEnv
    env = VecAoEnv(tc.params(tc.LAYERS_1), 4, RL, n_agents_modal=1, frame_pipeline=True)
    sup = env.supervisor
    fld = F.ScienceField(sup, F.line(20, 3))
    env.reset()
    zero = torch.zeros(4, env.action_dim, device=DEV)
    for _ in range(3):
        env.step(zero)
    assert sup.sim.frame_pipeline_state()[0], "no pipelined frame in flight: this test needs one"
    with pytest.raises(RuntimeError, match="ScienceField.observe: a pipelined frame is in flight"):
        fld.observe()
    nat, sim = fld.native, sup.sim
    assert nat.lib.aomarl_field_observe(nat.handle, sim.ctx, C.byref(sim.st), 0, 4, 3, nat._stream()) == 1
    with pytest.raises(la.AomarlError, match="field_observe: the frame pipeline is on"):
        la.check(1)
    assert float(fld.record.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 6. closed loop
def test_closed_loop_strehl_falls_with_the_field_angle(loop):
    """One layer at 8000 m, 4 environments x 100 integrator frames: the long-exposure Strehl along line(20, 5) is
    non-increasing within the spread between the environments and strictly lower at 20 arcsec than on axis.  Every
    direction and every environment counts.  (On the CPU path with 30 frames: tests/test_field.py.)"""
    sup = loop
    fld = F.ScienceField(sup, F.line(20, 5))
    sup.reset()
    le = fld.run(100)[..., 1].cpu().numpy()
    assert le.shape == (4, 5)
    mean, spread = le.mean(0), le.max(0) - le.min(0)
    print("long-exposure Strehl at 0, 5, 10, 15, 20 arcsec: %s; spread between the environments %s; the loop's own %.4f" % (
        np.array2string(mean, precision=4), np.array2string(spread, precision=4), float(sup.get_strehl()[:, 1].mean())))
    assert np.all(mean[1:] <= mean[:-1] + np.maximum(spread[1:], spread[:-1]))
    assert mean[4] < mean[0] and np.all(le[:, 4] < le[:, 0])
