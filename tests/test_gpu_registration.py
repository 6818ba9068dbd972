"""Mirror mis-registration on the device (csrc/aomarl_capi_dmreg.hip: k_trace_reg, through ao_marl_amd/registration.py)
against the existing trace, against the float64 model (registration.trace_model) fed the device's own planes, its
determinism, and the closed loop of the 10x10 system with a registration attached.

Tolerances.  Identity table: the bits of aomarl_raytrace_wfs / _target (the same expressions in the same order).  Whole
pixel shifts and quarter turns: the bits of the model in float32 (no product is involved: the cell's value, added).
Fractional maps: the yardstick is float64; the allowance is 4 x the deviation of the SAME model in float32 NumPy on the
CPU, measured by the test at run time (the project's convention for fp32 kernels, tests/test_gpu_pyramid.py).  Every
test prints its figures before it asserts.  The parameter sets are tests/registration_cases.py (conditioning proved on
the CPU by tests/test_registration.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import registration as R  # noqa: E402
from tests import registration_cases as rc  # noqa: E402

DEV = "cuda:0"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)
GRID = {False: "wfs", True: "tar"}


@pytest.fixture(scope="module")
def sup():
    from ao_marl_amd.env import VecRlSupervisor
    return VecRlSupervisor(rc.NAME, RL, rc.NENV, device=DEV)


@pytest.fixture(scope="module")
def rig(sup):
    """a simulator of its own on the supervisor's system: screens a few frames behind a reset, every mirror on a random
    command of its own per environment; (sim, table, planes [ndm][nenv, dim, dim] as the device evaluates them)"""
    from ao_marl_amd.sim import HipSim
    sim = HipSim(sup.s, nenv=rc.NENV, device=DEV, keep_phase=True)
    sim.reset(1234 + 16 * np.arange(rc.NENV))
    for _ in range(3):
        sim.move_atmos()
    g = torch.Generator().manual_seed(11)
    volts = 30.0 * torch.randn(rc.NENV, sup.s.nactu, generator=g)       # 0.01 um / V: a few tenths of a micron
    volts[:, -2:] *= 4.0                                                 # (tip-tilt: 0.003 um per unit at the edge)
    sim.comp_dm_shape(volts.to(DEV))
    planes = [sim.dm_shape(k).cpu().numpy() for k in range(len(sup.s.dms))]
    assert tuple(p.shape[1] for p in planes) == rc.DIMS and all(np.abs(p).max() > 0.05 for p in planes)
    return sim, R.NativeRegistration(sim), planes


def _buf(sim, target):
    return sim.t["tar_phase" if target else "wfs_phase"]


def _plain(sim, target, **kw):
    (sim.raytrace_target if target else sim.raytrace_wfs)(**kw)


def _set(reg, rows):
    for k in range(rows.shape[0]):
        reg.set_rows(k, rows[k])


# ------------------------------------------------------------------------------------------------ 1. identity table
@pytest.mark.parametrize("target", [False, True])
def test_identity_table_is_the_existing_trace(rig, target):
    sim, reg, _ = rig
    _set(reg, np.tile(R.IDENTITY_ROW, (2, rc.NENV, 1)))
    buf = _buf(sim, target)
    fill = torch.randn(buf.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    for atm, dms, reset in ((True, True, True), (False, True, True), (False, True, False)):
        buf.copy_(fill)
        _plain(sim, target, atm=atm, dms=dms, reset=reset)
        want = buf.clone()
        buf.copy_(fill)
        reg.trace(target, atm=atm, dms=dms, reset=reset)
        diff = (buf - want).abs().max().item()
        print("identity, %s, atm %d dms %d reset %d: largest |difference| %.3e of |phase| %.3e" %
              (GRID[target], atm, dms, reset, diff, want.abs().max().item()))
        assert torch.equal(buf, want) and want.abs().max() > 0.05
        assert not torch.equal(want, fill)


# ------------------------------------------------------------------------------------------------ 2. exact cases
@pytest.mark.parametrize("name", ["integer", "quarter"])
def test_exact_cases_equal_the_model(rig, name):
    sim, reg, planes = rig
    rows = rc.CASES[name]()
    _set(reg, rows)
    for target in (False, True):
        nn, offsets = rc.GRIDS[GRID[target]]
        reg.trace(target, atm=False, dms=True, reset=True)
        got = _buf(sim, target).cpu().numpy()
        for e in range(rc.NENV):
            want = R.trace_model(nn, [p[e] for p in planes], offsets, rows[:, e], dtype=np.float32)
            assert want.dtype == np.float32 and np.abs(want).max() > 0.05 and (want == 0).any()
            assert np.array_equal(got[e], want), (name, GRID[target], e, np.abs(got[e] - want).max())


# ------------------------------------------------------------------------------------------------ 3. fractional cases
@pytest.mark.parametrize("target", [False, True])
def test_fractional_case_against_float64(rig, target):
    """shift, rotation and magnification mixed, another set per environment and mirror in ONE launch, the atmosphere's
    part in front (the device's own, from a trace of the layers alone)"""
    sim, reg, planes = rig
    rows = rc.CASES["fractional"]()
    _set(reg, rows)
    nn, offsets = rc.GRIDS[GRID[target]]
    _plain(sim, target, atm=True, dms=False, reset=True)
    atmos = _buf(sim, target).cpu().numpy()
    reg.trace(target, atm=True, dms=True, reset=True)
    got = _buf(sim, target).cpu().numpy().astype(np.float64)
    e_dev, e_cpu, top = 0.0, 0.0, 0.0
    for e in range(rc.NENV):
        pl = [p[e] for p in planes]
        m64 = R.trace_model(nn, pl, offsets, rows[:, e], dtype=np.float64, start=atmos[e])
        m32 = R.trace_model(nn, pl, offsets, rows[:, e], dtype=np.float32, start=atmos[e])
        e_dev, e_cpu = max(e_dev, np.abs(got[e] - m64).max()), max(e_cpu, np.abs(m32.astype(np.float64) - m64).max())
        top = max(top, np.abs(m64).max())
        assert np.abs(m64 - atmos[e]).max() > 0.05              # the mirrors are in it
    print("fractional, %s: device - float64 %.3e   CPU float32 - float64 %.3e   (largest |phase| %.3e)" %
          (GRID[target], e_dev, e_cpu, top))
    assert e_cpu > 0 and e_dev <= 4 * e_cpu, (e_dev, e_cpu)


# ------------------------------------------------------------------------------------------------ 4. ranges and reruns
def test_ranges_reruns_and_get(rig):
    sim, reg, _ = rig
    rows = rc.CASES["fractional"]()
    _set(reg, np.tile(R.IDENTITY_ROW, (2, rc.NENV, 1)))
    reg.set_rows(0, rows[0, :1], env_begin=0)                   # the table in pieces, env_begin != 0 among them
    reg.set_rows(0, rows[0, 1:], env_begin=1)
    reg.set_rows(1, rows[1, 2:], env_begin=2)
    reg.set_rows(1, rows[1, :2])
    for k in range(2):
        assert np.array_equal(reg.get_rows(k), rows[k])
        assert np.array_equal(reg.get_rows(k, env_begin=1, env_count=2), rows[k, 1:3])
    for target in (False, True):
        buf = _buf(sim, target)
        buf.zero_()
        reg.trace(target, env_begin=0, env_count=3)
        whole = buf.clone()
        assert whole[:3].abs().max() > 0.05 and not whole[3].any()
        buf.zero_()
        reg.trace(target, env_begin=0, env_count=1)
        reg.trace(target, env_begin=1, env_count=2)
        assert torch.equal(buf, whole)
        buf.zero_()
        reg.trace(target, env_begin=0, env_count=3)
        assert torch.equal(buf, whole)
    from ao_marl_amd.libaomarl import AomarlError
    with pytest.raises(AomarlError, match="environments"):
        reg.trace(False, env_begin=2, env_count=3)
    with pytest.raises(AomarlError, match="det A"):
        reg.set_rows(0, np.array([[1, 1, 1, 1, 0, 0]], dtype=np.float32))
    with pytest.raises(AomarlError, match="mirror"):
        reg.set_rows(2, rows[0])
    assert np.array_equal(reg.get_rows(0), rows[0])             # a refused set leaves the table alone


# ------------------------------------------------------------------------------------------------ 5. loop, identity
def _frames(sup, n, part_one):
    out = []
    sup.reset()
    for _ in range(n):
        part_one()
        out.append((sup.get_slopes().clone(), sup.get_command().clone()))
        sup.next_part_two(None, linear_control=True)
    return out, sup.get_strehl().clone()


def _unfused_part_one(sup):
    """the frame of VecRlSupervisor.next_part_one through the existing unfused calls"""
    def run():
        sim = sup.sim
        sup.materialize_control()
        sim.move_atmos()
        sim.raytrace_target(atm=True, dms=True, reset=True)
        sim.target_psf_buffer()
        sim.raytrace_wfs(atm=True, dms=True, reset=True)
        sim.comp_image(from_phase_buffer=True, noise=True, write_bincube=False, cog=True)
        if sup.prefetch_atmos:
            sim.prefetch_atmos()
        sim.do_control()
        sup.iter += 1
    return run


def test_loop_with_the_identity_table(sup):
    from ao_marl_amd.env import VecRlSupervisor
    reg = R.DmRegistration(sup)
    reg.start()
    assert sup.registration is reg
    got, sr_got = _frames(sup, 20, sup.next_part_one)
    reg.stop()
    assert sup.registration is None
    want, sr_want = _frames(sup, 20, _unfused_part_one(sup))
    for f, ((s0, c0), (s1, c1)) in enumerate(zip(got, want)):
        assert torch.equal(s0, s1) and torch.equal(c0, c1), f
    assert torch.equal(sr_got, sr_want)
    assert got[-1][0].abs().max() > 0 and got[-1][1].abs().max() > 0 and not torch.equal(got[3][1], got[4][1])
    # after stop(): the supervisor is the one it was
    fresh = VecRlSupervisor(rc.NAME, RL, rc.NENV, device=DEV)
    a, sr_a = _frames(sup, 8, sup.next_part_one)
    b, sr_b = _frames(fresh, 8, fresh.next_part_one)
    for (s0, c0), (s1, c1) in zip(a, b):
        assert torch.equal(s0, s1) and torch.equal(c0, c1)
    assert torch.equal(sr_a, sr_b)


def test_keep_wfs_phase_is_the_registered_phase(sup):
    reg = R.DmRegistration(sup)
    reg.set(0, dx=0.5 * rc.PITCH * rc.PIXSIZE, theta=[0.0, 0.01, -0.01, 0.02])
    keep = sup.keep_wfs_phase
    sup.keep_wfs_phase = True
    try:
        reg.start()
        sup.reset()
        for _ in range(3):
            sup.next_part_one()
            seen = sup.get_wfs_phase().clone()
            assert torch.equal(seen, sup.sim.t["wfs_phase"])
            sup.next_part_two(None, linear_control=True)
        assert seen.abs().max() > 0
    finally:
        reg.stop()
        sup.keep_wfs_phase = keep


# ------------------------------------------------------------------------------------------------ 6. loop, shifted
def _variance(sup, nframes=300, first=100):
    """science-path phase variance per environment, mean over the frames first .. nframes"""
    sup.reset()
    acc = torch.zeros(sup.nenv, dtype=torch.float64, device=DEV)
    sup.next_part_one()
    for f in range(nframes):
        sup.next_part_two(None, linear_control=True)
        if f >= first:
            acc += sup.sim.t["strehl"][:, 2].double()
        sup.next_part_one()
    return (acc / (nframes - first)).cpu().numpy()


def test_loop_with_a_shifted_mirror():
    """Four environments on ONE seed.  Half an actuator pitch of shift costs phase variance; the command matrix
    calibrated through the shifted mirror wins it back.  Only the orderings are asserted."""
    from ao_marl_amd.env import VecRlSupervisor
    sup = VecRlSupervisor(rc.NAME, RL, 4, device=DEV, seed_stride=0)
    nominal = np.array(sup.s.cmat, dtype=np.float32)
    half = 0.5 * rc.PITCH * rc.PIXSIZE
    reg = R.DmRegistration(sup)
    reg.set(0, dx=[0.0, half, 0.25 * half, 0.0], theta=[0.0, 0.0, 0.0, np.deg2rad(1.0)])
    reg.start()
    mixed = _variance(sup)
    print("phase variance, frames 100-300, nominal matrix: registered %.5f  half a pitch %.5f  an eighth %.5f  one degree "
          "%.5f" % tuple(mixed))
    assert mixed[1] > mixed[0]
    reg.stop()
    reg.set(0, dx=half, theta=0.0)
    shape_before, table_before = sup.sim.dm_shape(0).clone(), reg.params["rows"]
    recal = reg.calibrate(env=0)
    assert recal.shape == nominal.shape and np.isfinite(recal).all() and not np.array_equal(recal, nominal)
    # the mirrors are back on the loop's voltages, the table is as it was, nothing was installed
    assert shape_before.abs().max() > 0 and torch.equal(sup.sim.dm_shape(0), shape_before)
    assert np.array_equal(reg.params["rows"], table_before) and np.array_equal(np.array(sup.s.cmat), nominal)
    reg.start()
    all_nominal = _variance(sup)
    R.install_cmat(sup, recal)
    all_recal = _variance(sup)
    reg.stop()
    R.install_cmat(sup, nominal)
    print("all shifted by half a pitch: nominal matrix %s  recalibrated %s" % (all_nominal, all_recal))
    assert (all_recal < all_nominal).all()
