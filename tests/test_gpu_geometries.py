"""The Shack-Hartmann chain on the geometries of tests/geometry_cases.py: every stage tests/test_gpu_parity.py compares
for the 10x10 production system (the shared code is tests/parity_stages.py), for six systems with odd tile counts,
pupils that are no multiple of 32 pixels, two layers, off-axis guide stars and targets (bilinear ray-trace), a mirror
at altitude, screens of several sizes on both sides of MOVE_SMALL_DIM.  Three environments: a partial group of four
per frame workgroup.  Nothing here builds the 40x40 system.

Which case reaches which branch (the library's own reports are asserted in the tests named):

  odd7         frame_fused_available() and dm_from_voltage_available() are asserted, frame_kernel_name() starts
               "k_frame_wave<1," (test_fused_frame): the 2 g + 1 < nt arm of pair_info, stripe_order / lit_info with
               nt = 7; k_target_rows_fast<1> and both other row kernels at pd % 64 = 48, npsf 256; k_move_small with
               ldt 128; k_transpose_ring / k_extrude_sg at n = 120, ns = 246.
  odd17        the same with "k_frame_wave<3,", nt = 17, pd % 64 = 16, npsf 1024, n = 280, ns = 571 (general move).
  off9         two layers, sensor and target fractional: bilinear_ring in k_raytrace (ring origin 0 and != 0), the
               composite's raytrace_wfs + FROM_PHASE_BUFFER route, k_target_rows_mfma<true> / k_target_rows<true>;
               two [A|B] classes (152, 190) in one small move; frame_fused() answers "geometry not eligible"
               (test_fused_frame); VecAoEnv leaves the frame pipeline on its own (test_env_step_matches_the_oracle_env).
  tar9         the mixed case: comp_image straight from the screens (k_wfs_spot<false>, two layers), PSF from the
               phase buffer; screens 152 / 218: k_move_small with ldt 192 and 256.
  off13        three layers 216 / 238 / 286: small_ok is false although two layers are small (the general move with
               three [A|B] classes), `small_move` 0 and 1 give the same screens.
  off13_dmalt  the interpolating branch of trace_dms (stack-array mirror at 3000 m, offsets 61.82 / 59.49).

All six tile counts are odd (7, 9, 9, 13, 13, 17); only odd7 and odd17 read the pair table (fused frame).

Bounds: those of test_gpu_parity.py where it checks the same stage; ray-trace against float64
8 * 2^-24 * (sum of max |screen| + sum of max |shape|) (geometry_cases.raytrace_bound); slopes, Strehl ratio and phase
variance against float64 1e-4 arcsec, 2e-5 SR + 1e-7, 1e-4 relative (tests/test_gpu_phase_range.py, no offset).

No case needed the "3 x the oracle's own distance" rule: every stage meets its parity bound on every case.

Measured on the MI355X (worst over the three seeds and the variants of a stage; "oracle" = the oracle's own distance
from the same float64 reference; also in LAB_NOTEBOOK.md):

  case         reset    7 moves | ray-trace - f64 (um)        | image    slopes - f64 (arcsec) | SR - f64 (rel)    var - f64 (rel)   | loop
               (um)     (um)    | kernel   oracle   of bound  | (of max) kernel   oracle       | kernel   oracle   kernel   oracle   | slopes
  odd7         3.0e-5   4.1e-6  | 2.4e-7   2.4e-7   0.16      | 4.9e-7   5.4e-7   2.3e-6       | 3.2e-7   3.5e-7   7.2e-8   2.3e-8   | 8.6e-6
  off9         2.8e-5   5.0e-6  | 4.2e-7   4.3e-7   0.17      | 6.3e-7   6.9e-7   2.1e-6       | 6.0e-7   3.2e-7   7.2e-8   3.9e-8   | 5.8e-6
  tar9         1.8e-5   5.2e-6  | 6.6e-7   6.6e-7   0.22      | 9.7e-7   5.0e-7   2.2e-6       | 6.9e-7   2.3e-7   1.1e-7   5.1e-8   | 6.0e-6
  off13        1.0e-4   1.1e-5  | 7.1e-7   7.4e-7   0.16      | 9.5e-7   6.0e-7   2.3e-6       | 3.8e-7   3.4e-7   9.3e-8   4.5e-8   | 1.0e-5
  off13_dmalt  1.0e-4   1.1e-5  | 7.6e-7   7.7e-7   0.24      | 1.0e-6   6.3e-7   2.5e-6       | 3.5e-7   3.3e-7   8.3e-8   3.9e-8   | 1.2e-5
  odd17        1.4e-4   1.6e-5  | 1.6e-6   1.6e-6   0.58      | 1.2e-6   8.3e-7   3.4e-6       | 1.7e-6   6.7e-7   0        3.2e-8   | 1.2e-5

(bounds: reset 2e-4, moves 2e-5, ray-trace 1.0 of its bound, image 2e-5, slopes 1e-4, SR 2e-5, variance 1e-4, loop
slopes 1e-4.)  Every fused mode of odd7 and odd17 chose NB = 1; dm_from_voltage_available() is true for both.  The
environment (10 steps, off9 and odd7): states within 2.0e-5, rewards 2.7e-5, slopes 4.1e-6 arcsec, commands 2.7e-6."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import aoref  # noqa: E402
from tests import geometry_cases as gc  # noqa: E402
from tests import helpers  # noqa: E402
from tests import parity_stages as stages  # noqa: E402

SEEDS = [1234, 1250, 77]            # nenv = 3: a partial group of four environments per frame workgroup
NAMES = list(gc.CASES)
FUSED = ("odd7", "odd17")
NFRAMES = 40


class _Setup(object):
    def __init__(self, name):
        from ao_marl_amd.sim import HipSim
        self.name = name
        self.sysm, self.s, self.cal = helpers.calibrated_params("geometry_case_" + name, lambda: gc.param_set(name))
        gc.assert_facts(gc.CASES[name], self.s)
        self.sim = HipSim(self.s, nenv=len(SEEDS), keep_bincube=True, keep_phase=True)
        self.sim.set_modal(self.cal.volts2modes, self.cal.modes2volts)
        self.sim.reset(SEEDS)
        self.oracles = [aoref.OracleSim(self.s, seed=sd) for sd in SEEDS]
        self.el = gc.eligibility(self.s)
        self._trace = None

    def trace(self):
        """The oracles' 40 closed-loop frames and the open-loop Strehl ratios: once per case, for both precisions."""
        if self._trace is None:
            self._trace = stages.OracleTrace(self.oracles, SEEDS, NFRAMES)
        return self._trace


@pytest.fixture(scope="module", params=NAMES)
def setup(request):
    st = _Setup(request.param)
    yield st
    del st.sim


def test_library_agrees_with_the_eligibility_rules(setup):
    sim, el = setup.sim, setup.el
    assert sim.frame_fused_available() == el["fused_ok"] == (setup.name in FUSED)
    if not el["fused_ok"]:
        assert not sim.dm_from_voltage_available()


def test_reset_screens_match_oracle(setup):
    print("%s reset: worst |screen - oracle| = %.3g um" % (setup.name, stages.check_reset_screens(setup.sim, setup.oracles)))


def test_move_atmos_matches_oracle(setup):
    """7 moves from the pushed oracle state with the small-system move kernel allowed (`small_move` 1, the default: it
    runs where every layer is small) and with the general chain (0): the oracle's screens, accumulators and extrusion
    counters both times, and the same screens to rounding (the bound of either against the oracle)."""
    sim, s, oracles = setup.sim, setup.s, setup.oracles
    start = [([scr.copy() for scr in o.screens], list(o.ext_count), o.accumx.copy(), o.accumy.copy()) for o in oracles]
    got = {}
    for small_move in (1, 0):
        for o, (scr, cnt, ax, ay) in zip(oracles, start):          # both runs from the same state
            for l in range(s.nscreens):
                o.screens[l][:] = scr[l]
            o.ext_count, o.accumx, o.accumy = list(cnt), ax.copy(), ay.copy()
        sim.set_option("small_move", small_move)
        try:
            worst = stages.check_moves(sim, oracles, nmoves=7)
        finally:
            sim.set_option("small_move", 1)
        got[small_move] = [sim.screen(l).cpu().numpy() for l in range(s.nscreens)]
        print("%s small_move=%d: worst |screen - oracle| after 7 moves = %.3g um" % (setup.name, small_move, worst))
    for l in range(s.nscreens):
        assert np.abs(got[0][l] - got[1][l]).max() < 2e-5, l


@pytest.mark.parametrize("generic", [0, 1])
def test_dm_shape_matches_oracle(setup, generic):
    stages.check_dm_shape(setup.sim, setup.oracles, generic)


@pytest.mark.parametrize("moved", [False, True])
def test_raytrace_matches_float64(setup, moved):
    """raytrace_wfs / raytrace_target against the float64 ray-trace of the screens and mirror shapes READ BACK from the
    device, and against the oracle on the same fields; ring origin 0 (pushed state), and behind a reset and 5 moves
    (origin != 0: the interpolation crosses the ring seam and the mirror columns)."""
    s, sim = setup.s, setup.sim
    if moved:
        sim.reset(SEEDS)
        for _ in range(5):
            sim.move_atmos()
        assert int(sim.t["origin"].abs().sum()) > 0
    else:
        stages.push_oracle_state(sim, setup.oracles)
        assert int(sim.t["origin"].abs().sum()) == 0
    rng = np.random.default_rng(13)
    volts = rng.normal(0, 50.0, size=(len(SEEDS), s.nactu)).astype(np.float32)       # mirrors of about half a micron
    volts[:, -2:] = rng.normal(0, 100.0, size=(len(SEEDS), 2))
    sim.comp_dm_shape(torch.from_numpy(volts).cuda())
    screens = [sim.screen(l).cpu().numpy() for l in range(s.nscreens)]
    shapes = [sim.dm_shape(k).cpu().numpy() for k in range(len(s.dms))]
    tracer = helpers.CalSim(s)
    worst = {}
    for target in (False, True):
        for atm, dms in ((True, True), (True, False), (False, True)):
            (sim.raytrace_target if target else sim.raytrace_wfs)(atm=atm, dms=dms, reset=True)
            got = sim.t["tar_phase" if target else "wfs_phase"].cpu().numpy()
            for e in range(len(SEEDS)):
                scr, shp = [a[e] for a in screens], [a[e] for a in shapes]
                ref = gc.raytrace64(s, scr, shp, target, atm=atm, dms=dms)
                bound = gc.raytrace_bound(scr if atm else [], shp if dms else [])
                d = float(np.abs(got[e] - ref).max())
                for l in range(s.nscreens):
                    tracer.screens[l][:] = scr[l]
                for k in range(len(s.dms)):
                    tracer.dm_shapes[k][:] = shp[k]
                (tracer.raytrace_target if target else tracer.raytrace_wfs)(atm=atm, dms=dms, reset=True)
                oph = tracer.tar_phase if target else tracer.wfs_phase
                key = ("tar" if target else "wfs", atm, dms)
                w = worst.setdefault(key, [0.0, 0.0, 0.0, bound])
                w[0], w[1] = max(w[0], d), max(w[1], float(np.abs(oph - ref).max()))
                w[2] = max(w[2], float(np.abs(got[e] - oph).max()))
                assert np.abs(ref).max() > 0.05
                assert d <= bound, (setup.name, key, e, d, bound)
                assert np.abs(got[e] - oph).max() < 1e-5, (setup.name, key, e)
    for key, w in worst.items():
        print("%s moved=%d %s atm=%d dms=%d: kernel - float64 %.3g, oracle - float64 %.3g, kernel - oracle %.3g (bound %.3g)"
              % ((setup.name, moved) + key + tuple(w)))


@pytest.mark.parametrize("generic", [0, 1])
def test_spots_and_slopes_match_oracle_and_float64(setup, generic):
    """The image from the phase buffer in every case, straight from the screens where the sensor's offsets are
    integers, both spot kernels, slopes only, stand-alone do_centroids; slopes against slopes64 of the read-back phase."""
    w = stages.check_raytrace_and_spots(setup.sim, setup.oracles, generic, ref64=True)
    print("%s generic_spot=%d: phase %.3g um, image %.3g of max, slopes - oracle %.3g, slopes - float64 %.3g, "
          "oracle - float64 %.3g arcsec" % (setup.name, generic, w["phase"], w["image"], w["slopes"], w["slopes64"], w["oracle64"]))


@pytest.mark.parametrize("valu", [0, 1, 2])
def test_target_psf_and_strehl_match_oracle_and_float64(setup, valu):
    w = stages.check_target_psf(setup.sim, setup.oracles, valu, ref64=True)
    print("%s rows=%d: phase %.3g um; SR - oracle %.3g, var - oracle %.3g; SR - float64 %.3g, var - float64 %.3g; oracle - "
          "float64: SR %.3g, var %.3g (relative)" % (setup.name, valu, w["phase"], w["strehl"], w["var"], w["strehl64"],
                                                     w["var64"], w["oracle_sr64"], w["oracle_var64"]))


def test_fused_frame(setup):
    """odd7 / odd17: the six modes of test_gpu_parity.py::test_fused_frame_matches_oracle_and_unfused.  The other four:
    frame_fused() is refused with the library's message and launches nothing."""
    from ao_marl_amd import libaomarl as la
    sim, s = setup.sim, setup.s
    if setup.name not in FUSED:
        assert not sim.frame_fused_available()
        stages.push_oracle_state(sim, setup.oracles)
        sim.slopes.fill_(7.0)
        before = dict(la.arith_launches())
        with pytest.raises(la.AomarlError, match="geometry not eligible"):
            sim.frame_fused(noise=False, write_bincube=False, cog=True, dm_from_voltage=False)
        torch.cuda.synchronize()
        assert dict(la.arith_launches()) == before and bool((sim.slopes == 7.0).all())
        return
    assert sim.frame_fused_available()
    otf = sim.dm_from_voltage_available()
    names = stages.check_fused_frame(sim, setup.oracles, otf=otf)
    nl = 1 if setup.name == "odd7" else 3
    assert set(names) == set(m for m in stages.FRAME_MODES[1:] if otf or not m.startswith("otf"))
    for mode, nm in names.items():
        assert nm.startswith("k_frame_wave<%d, " % nl), (mode, nm)
        print("%s %s: %s (NB = %s)" % (setup.name, mode, nm, nm.split(",")[1].strip()))
    if not otf:
        assert not sim.dm_from_voltage_available()
        print("%s: dm_from_voltage_available() is false, the otf modes did not run" % setup.name)


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
def test_closed_loop_trace_matches_oracle(setup, precision):
    """40 frames of next_part_two + next_part_one from a common pushed state, in the default precision and with the
    DFTs and internal GEMMs on split-fp16 MFMAs: the one-pass frame kernel (odd7, odd17), the composite's separate
    passes -- ray-trace + FROM_PHASE_BUFFER where an offset is fractional -- for the others.  The loop closes: the
    short-exposure Strehl ratio, averaged over the second half of the trace and the three seeds, lies above the
    OPEN-loop one of the same screens (the oracle's atmosphere, flat mirrors, float64), for the kernels and for the
    oracle itself -- what off-axis anisoplanatism leaves to assert (a single seed may lose: the oracle's seed 77 of
    off13_dmalt closes at 0.38 against 0.41 open loop, 11 arcsec between guide star and target; its mean over the
    seeds is 0.53 against 0.29).  On axis (odd7, odd17) every seed must win."""
    sim = setup.sim
    trace = setup.trace()
    launched, worst, se = stages.closed_loop(sim, None, SEEDS, precision, nframes=NFRAMES, trace=trace)
    fused = setup.name in FUSED
    if precision == "f32":
        assert not any("split" in k for k in launched), launched
    else:
        assert launched.get("gemm:split_f16_mfma", 0) > 0, launched
        assert launched.get("frame_kernel_dft:split_f16_mfma", 0) == (NFRAMES if fused else 0), launched
    if fused:
        assert sim.frame_kernel_name().startswith("k_frame_wave<%d, " % (1 if setup.name == "odd7" else 3))
    half = NFRAMES // 2
    closed, opened = se[half:].mean(axis=0), trace.open_loop[half:].mean(axis=0)
    oracle_closed = np.array([[f.strehl_se for f in row] for row in trace.frames[half:]]).mean(axis=0)
    print("%s %s: worst slope deviation %.3g arcsec; SE Strehl, frames %d-%d: closed %s (oracle %s), open loop %s"
          % (setup.name, precision, worst, half, NFRAMES, closed, oracle_closed, opened))
    assert oracle_closed.mean() > opened.mean() and closed.mean() > opened.mean(), (closed, oracle_closed, opened)
    if fused:
        assert (closed > opened).all(), (closed, opened)


def test_calibration_through_hip_backend_matches_oracle_backend(setup):
    """modal.calibrate through HipSim.dm_response (what VecAoEnv does) against the oracle-backed calibration of the
    fixture, with test_gpu_parity.py's bounds.  Off axis the sensor's layer offsets are fractional: the response goes
    through raytrace_wfs + the phase buffer (comp_image refuses to trace such a path itself)."""
    from ao_marl_amd import geometry as G, modal, system
    from ao_marl_amd.sim import HipSim
    cal_o = setup.cal
    sysm = G.build_system(gc.param_set(setup.name))
    s = system.from_system(sysm, strehl_halfwin=8)
    backend = HipSim(s, nenv=64, keep_phase=True)
    cal = modal.calibrate(s, sysm, backend, nfilt=5, cache=False)
    assert [len(k) for k in cal.kept] == [len(k) for k in cal_o.kept]
    assert np.array_equal(cal.kept[0], cal_o.kept[0])      # same actuators survive, exactly
    assert np.abs(cal.imat - cal_o.imat).max() < 1e-4 * np.abs(cal_o.imat).max()
    assert np.abs(cal.cmat - cal_o.cmat).max() < 2e-3 * np.abs(cal_o.cmat).max()
    assert np.abs(cal.Btt - cal_o.Btt).max() < 1e-6


# ------------------------------------------------------------------------------------------------ the environment
ENV_STEPS = 10
ENV_RL = dict(n_zernike_start_end=[0, 40], n_reverse_filtered_from_cmat=5)


def _env_norm(nslope, nmodes):
    """Standardisation statistics and action bounds for a system the reference never recorded any for: zero means,
    one scale per block (the two sides divide by the same numbers)."""
    def block(n, sd):
        return dict(mean=np.zeros(n, np.float32), std=np.full(n, sd, np.float32), max=np.full(n, 10 * sd, np.float32),
                    min=np.full(n, -10 * sd, np.float32))
    return (dict(wfs=block(nslope, 0.1), dm=block(nmodes, 0.5), dm_residual=block(nmodes, 0.05)),
            np.full(nmodes, 0.05, np.float32))


@pytest.mark.parametrize("pipeline", [False, True])
@pytest.mark.parametrize("name", ["off9", "odd7"])
def test_env_step_matches_the_oracle_env(monkeypatch, name, pipeline):
    """VecAoEnv with its default settings (one modal agent + the tip-tilt agent) through aomarl_env_step for 10 steps
    against the same host logic over the CPU oracle, as tests/test_gpu_env_step_large.py does for the 40x40 system,
    with its bounds.  pipeline: a frame in flight where the loop is eligible -- odd7 flies, off9 (no fused frame)
    takes the plain order on its own."""
    import copy
    from ao_marl_amd import geometry as G, modal, system
    from ao_marl_amd.env import VecAoEnv
    from tests import test_gpu_env_step_large as large
    nenv = len(SEEDS)
    PushedSim = large._pushed_sim_class()
    PushedSim.reset_limit = 2e-4               # test_gpu_parity.py's bound for the reset of a small system
    _, _, s0 = gc.build(name)
    nmodes = setup_nmodes = helpers.calibrated_params("geometry_case_" + name, lambda: gc.param_set(name))[2].volts2modes.shape[0]
    norm, zn = _env_norm(s0.nslope, nmodes)
    kw = dict(initial_seed=1234, seed_stride=16, n_agents_modal=1, norm=norm, zn_norm=zn)
    env = VecAoEnv(gc.param_set(name), nenv, ENV_RL, device="cuda:0", sim_factory=PushedSim, frame_pipeline=pipeline, **kw)
    assert env.nmodes == setup_nmodes and env.layout.n_agents == 2
    assert env._native_glue and env._default_state_layout
    cal = env.supervisor.cal

    def calibrate(s, sysm, backend, nfilt=0, verbose=False, **kwargs):
        for k, d in enumerate(s.dms):
            if d.type == "pzt":
                G.pzt_select(d, sysm.geom, cal.kept[k])
        system.refresh_dms(s)
        s.cmat = np.ascontiguousarray(cal.cmat)
        return copy.copy(cal)
    monkeypatch.setattr(modal, "calibrate", calibrate)
    oenv = VecAoEnv(gc.param_set(name), nenv, ENV_RL, device="cpu", sim_factory=large.SnapOracleVecSim, **kw)
    monkeypatch.undo()
    assert oenv.supervisor.s.nactu == env.supervisor.s.nactu
    so = oenv.reset().numpy()
    PushedSim.source = oenv.supervisor.sim
    sg = env.reset()
    PushedSim.source = None
    assert sg.shape == (nenv, env.state_dim) == so.shape
    rng = np.random.default_rng(5)
    worst = dict(state=0.0, reward=0.0, slopes=0.0, com=0.0)
    used_native = 0
    for it in range(ENV_STEPS):
        d = np.abs(sg.cpu().numpy() - so).max() / np.maximum(1.0, np.abs(so).max())
        worst["state"] = max(worst["state"], d)
        assert d < 2e-3, ("state", it, d)
        used_native += int(env._native_step_ok(False))
        a = rng.uniform(-1, 1, size=(nenv, env.action_dim)).astype(np.float32)
        sg, rg, done, _ = env.step(torch.from_numpy(a).cuda())
        so_t, ro, _, _ = oenv.step(torch.from_numpy(a))
        so, ro, rg = so_t.numpy(), ro.numpy(), rg.cpu().numpy()
        assert rg.shape == ro.shape == (nenv, 2) and done is False
        dr = np.abs(rg - ro).max() / np.maximum(np.abs(ro).max(), 1e-12)
        worst["reward"] = max(worst["reward"], dr)
        assert dr < 2e-3, ("reward", it, dr)
        sl = env.supervisor.get_slopes().cpu().numpy()
        slo = oenv.supervisor.get_slopes().numpy()
        worst["slopes"] = max(worst["slopes"], np.abs(sl - slo).max())
        assert np.abs(sl - slo).max() < 1e-4, ("slopes", it)            # arcsec, the north-star tolerance
        cm = env.supervisor.get_command().cpu().numpy()
        cmo = oenv.supervisor.get_command().numpy()
        dc = np.abs(cm - cmo).max() / np.abs(cmo).max()
        worst["com"] = max(worst["com"], dc)
        assert dc < 5e-4, ("com", it, dc)
    assert used_native == ENV_STEPS                      # every step went through aomarl_env_step
    flying, _, piped, beside = env.supervisor.sim.frame_pipeline_state()
    fused = name in FUSED
    assert env.supervisor.sim.frame_fused_available() == fused
    assert (flying, piped, beside) == ((True, ENV_STEPS - 1, ENV_STEPS) if pipeline and fused else (False, 0, 0))
    if fused:
        assert env.supervisor.sim.frame_kernel_name().startswith("k_frame_wave<1, ")
    st = env.supervisor.get_strehl().cpu().numpy()
    sto = oenv.supervisor.get_strehl().numpy()
    assert np.abs(st[:, :2] - sto[:, :2]).max() < 2e-4
    print("%s pipeline=%s: worst deviations over %d steps %s; full reset against the oracle's screens %.2e um"
          % (name, pipeline, ENV_STEPS, worst, PushedSim.reset_diff))
