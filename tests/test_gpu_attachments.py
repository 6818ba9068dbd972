"""The frame of every sensing loop attachment (ao_marl_amd/attachments.py: pyramid, laser guide star, mirror
mis-registration) against its launch sequence spelled out here from the simulator's and the sensor's primitives: the
sequence VecRlSupervisor.next_part_one must issue, launch for launch (bit-equal slopes, err, command, voltages and
Strehl after every frame), and an environment that is, after stop(), the one that never had an attachment."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import params as P  # noqa: E402

DEV = "cuda:0"
NAME = "production_sh_10x10_2m"
RL = dict(n_zernike_start_end=[0, 80], n_reverse_filtered_from_cmat=5)      # (the agents' layout needs the range)
NENV, FRAMES = 2, 3


def _env():
    from ao_marl_amd.env import VecAoEnv
    return VecAoEnv(P.builtin(NAME), NENV, RL, n_agents_modal=1, frame_pipeline=False)


@pytest.fixture(scope="module")
def rig():
    """(environment, never-attached twin, {name: attachment on the environment's supervisor}): each sensor calibrated
    once, the registration a 0.3-pitch shift of mirror 0"""
    from ao_marl_amd.lgs import LgsSensor
    from ao_marl_amd.pyramid import PyramidSensor
    from ao_marl_amd.registration import DmRegistration
    env, twin = _env(), _env()
    sup = env.supervisor
    pyr = PyramidSensor(sup, nxsub=20)
    pyr.calibrate()
    lgs = LgsSensor(sup, gsalt=90e3, llt=(0., 0.))
    lgs.calibrate()
    reg = DmRegistration(sup)
    reg.set(0, dx=0.3 * float(sup.s.dms[0].pitch) * reg.pixsize)
    return env, twin, dict(pyramid=pyr, lgs=lgs, registration=reg)


def _own_control(sup, sen):
    sim = sup.sim
    sim.gemm_nt(sen.slopes, sen._cmat_dev, alpha=-1.0, beta=0.0, Cout=sim.err)
    sim.com.add_(sim.err, alpha=float(sup.gain))


def _pyramid_frame(sup, pyr):
    sim = sup.sim
    sim.move_atmos()
    sim.target_psf()
    sim.raytrace_wfs(atm=True, dms=True, reset=True)
    if sup.prefetch_atmos:
        sim.prefetch_atmos()
    pyr.measure()
    _own_control(sup, pyr)
    return pyr.slopes


def _lgs_frame(sup, lgs):
    sim = sup.sim
    sim.move_atmos()
    sim.target_psf()
    lgs.trace()
    if sup.prefetch_atmos:
        sim.prefetch_atmos()
    lgs.measure(write_cube=False)
    _own_control(sup, lgs)
    return lgs.slopes


def _registration_frame(sup, reg):
    sim = sup.sim
    sim.move_atmos()
    reg.trace(target=True)
    sim.target_psf_buffer()
    reg.trace(target=False)
    sim.comp_image(from_phase_buffer=True, noise=True, write_bincube=False, cog=True)
    if sup.prefetch_atmos:
        sim.prefetch_atmos()
    sim.do_control()
    return sim.slopes


SPELLED = dict(pyramid=_pyramid_frame, lgs=_lgs_frame, registration=_registration_frame)


def _run(sup, part_one):
    """reset (it restarts the seeds), then FRAMES x (next_part_two, part_one): what every frame leaves"""
    sup.reset()
    out = []
    for _ in range(FRAMES):
        sup.next_part_two(None, linear_control=True)
        slopes = part_one()
        out.append([t.clone() for t in (slopes, sup.get_err(), sup.get_command(), sup.get_voltages(), sup.get_strehl())])
    return out


@pytest.mark.parametrize("name", ["pyramid", "lgs", "registration"])
def test_next_part_one_issues_the_spelled_out_sequence(rig, name):
    env, _, atts = rig
    sup, att = env.supervisor, atts[name]
    assert not sup.keep_wfs_phase and getattr(sup.sim, "_twin", None) is None

    def supervisors():
        sup.next_part_one()
        return sup.get_slopes()

    def spelled():                              # the head and the tail of next_part_one around the attachment's frame
        sup._check_atmos_change()
        sup.materialize_control()
        sup._err_stale = False
        slopes = SPELLED[name](sup, att)
        sup.iter += 1
        return slopes
    att.start()
    try:
        assert getattr(sup, name) is att
        got = _run(sup, supervisors)
        want = _run(sup, spelled)
    finally:
        att.stop()
    assert getattr(sup, name) is None
    for f, (a, b) in enumerate(zip(got, want)):
        for what, x, y in zip(("slopes", "err", "command", "voltages", "strehl"), a, b):
            assert torch.equal(x, y), (f, what)
    assert got[-1][0].abs().max() > 0 and got[-1][2].abs().max() > 0 and not torch.equal(got[1][2], got[2][2])


def test_after_stop_the_environment_is_the_never_attached_one(rig):
    env, twin, atts = rig
    zero = torch.zeros(NENV, env.action_dim, device=DEV)
    act = 0.1 * torch.randn(NENV, env.action_dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    for name in ("pyramid", "lgs", "registration"):
        atts[name].start()
        try:
            assert not env._native_step_ok(False)
            env.reset()
            s, _, _, _ = env.step(zero, linear_control=True)
            assert torch.isfinite(s).all()
        finally:
            atts[name].stop()
        sa, sb = env.reset(), twin.reset()
        assert torch.equal(sa, sb), name
        (sa, ra, _, _), (sb, rb, _, _) = env.step(act), twin.step(act)
        assert torch.equal(sa, sb) and torch.equal(ra, rb), name
        assert torch.equal(env.supervisor.get_command(), twin.supervisor.get_command()), name
