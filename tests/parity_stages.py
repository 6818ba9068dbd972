"""Stage-by-stage comparisons of the HIP path with the CPU oracle, shared by tests/test_gpu_parity.py (the 10x10
production system) and tests/test_gpu_geometries.py (tests/geometry_cases.py).  Tolerances are fp32 round-off of
different summation orders / algorithms (pruned MFMA DFT vs padded FFT, ring buffer vs shift, fused vs materialised
raytrace); index-like outputs (brightest pixel) are exact.  The float64 comparisons (`ref64=True`) take the bounds of
tests/test_gpu_phase_range.py for phases that are not shifted: 1e-4 arcsec, 2e-5 SR + 1e-7, 1e-4 of the variance."""
import numpy as np
import torch

from tests import geometry_cases as gc
from tests import phase_range as pr

FRAME_MODES = ("unfused", "fused_cube", "fused", "otf_cube", "otf", "otf_f32")


def push_oracle_state(sim, oracles):
    """Copy the oracle's screens into the HIP state (origin 0) so later stages are compared on
    identical inputs."""
    s = sim.s
    for l, d in enumerate(s.screen_dim):
        sim.set_screen(l, np.stack([o.screens[l] for o in oracles]))
    for e, o in enumerate(oracles):
        sim.t["ext_count"][e] = torch.tensor(o.ext_count, dtype=torch.int32)
        sim.accumx[e] = o.accumx
        sim.accumy[e] = o.accumy


def all_int(offsets):
    return all(float(v).is_integer() for o in offsets for v in o)


def check_reset_screens(sim, oracles):
    s = sim.s
    worst = 0.0
    for l in range(s.nscreens):
        scr = sim.screen(l).cpu().numpy()
        for e, o in enumerate(oracles):
            d = np.abs(scr[e] - o.screens[l]).max()
            worst = max(worst, float(d))
            assert d < 2e-4, (l, e, d)   # 2n extrusions of fp32 recursion, screens ~ +-2 um
            assert np.std(o.screens[l]) > 0.05
    return worst


def check_moves(sim, oracles, nmoves=7):
    """`nmoves` frames of wind from the pushed oracle state: screens, accumulators and extrusion counters."""
    s = sim.s
    push_oracle_state(sim, oracles)
    for _ in range(nmoves):
        sim.move_atmos()
        for o in oracles:
            o.move_atmos()
    worst = 0.0
    for l in range(s.nscreens):
        scr = sim.screen(l).cpu().numpy()
        for e, o in enumerate(oracles):
            d = float(np.abs(scr[e] - o.screens[l]).max())
            worst = max(worst, d)
            assert d < 2e-5, (l, e, d)
    # the ring origin moved, the logical content did not wrap
    assert int(sim.t["origin"].abs().sum()) > 0
    cnt = sim.t["ext_count"].cpu().numpy()
    for e, o in enumerate(oracles):
        assert np.array_equal(sim.accumx[e], o.accumx)
        assert np.array_equal(sim.accumy[e], o.accumy)
        assert np.array_equal(cnt[e, :s.nscreens], np.asarray(o.ext_count)), (e, cnt[e], o.ext_count)
    return worst


def check_dm_shape(sim, oracles, generic, sigma=1.0):
    """Both stack-array kernels: the separable-lattice fast path and the generic gather over the
    reference's influpos tables."""
    s = sim.s
    rng = np.random.default_rng(3)
    volts = rng.normal(0, sigma, size=(len(oracles), s.nactu)).astype(np.float32)
    sim.set_option("force_generic_dm", generic)
    sim.comp_dm_shape(torch.from_numpy(volts).cuda())
    sim.set_option("force_generic_dm", 0)
    for e, o in enumerate(oracles):
        o.comp_shapes(volts[e])
        for k in range(len(s.dms)):
            a = sim.dm_shape(k)[e].cpu().numpy()
            assert np.abs(a - o.dm_shapes[k]).max() < 2e-6 * max(1.0, np.abs(o.dm_shapes[k]).max())


def check_raytrace_and_spots(sim, oracles, generic, ref64=False):
    """Unfused API (raytrace -> buffer -> image), and where the sensor's offsets are integers the kernels that read the
    screens themselves (software-pipelined fast variant and the generic one); stand-alone COG; slopes only.
    ref64: also the slopes against the float64 centre of gravity of the phase read back from the device."""
    s = sim.s
    direct = all_int(list(s.wfs_atm_off) + list(s.wfs_dm_off))
    sim.set_option("force_generic_spot", generic)
    push_oracle_state(sim, oracles)
    rng = np.random.default_rng(4)
    volts = rng.normal(0, 0.5, size=(len(oracles), s.nactu)).astype(np.float32)
    sim.comp_dm_shape(torch.from_numpy(volts).cuda())
    # unfused API: raytrace -> phase buffer -> image from buffer
    sim.raytrace_wfs(atm=True, dms=False, reset=True)
    sim.raytrace_wfs(atm=False, dms=True, reset=False)
    sim.comp_image(from_phase_buffer=True, noise=False, write_bincube=True, cog=True)
    cube_buf = sim.t["bincube"].cpu().numpy().copy()
    sl_buf = sim.slopes.cpu().numpy().copy()
    ph = sim.t["wfs_phase"].cpu().numpy()
    # fused path (the image kernel traces the screens itself)
    sim.comp_image(from_phase_buffer=not direct, noise=False, write_bincube=True, cog=True)
    cube_fused = sim.t["bincube"].cpu().numpy().copy()
    sl_fused = sim.slopes.cpu().numpy().copy()
    sim.slopes.zero_()
    sim.do_centroids()
    sl_cog = sim.slopes.cpu().numpy().copy()
    # slopes-only path (no bincube): single-pass reduction of the raw image
    sim.slopes.zero_()
    sim.comp_image(from_phase_buffer=not direct, noise=False, write_bincube=False, cog=True)
    sl_only = sim.slopes.cpu().numpy().copy()
    sim.set_option("force_generic_spot", 0)
    worst = dict(phase=0.0, image=0.0, slopes=0.0, slopes64=0.0, oracle64=0.0)
    for e, o in enumerate(oracles):
        o.comp_shapes(volts[e])
        o.raytrace_wfs(atm=True, dms=False, reset=True)
        o.raytrace_wfs(atm=False, dms=True, reset=False)
        worst["phase"] = max(worst["phase"], float(np.abs(ph[e] - o.wfs_phase).max()))
        assert np.abs(ph[e] - o.wfs_phase).max() < 1e-5
        o.comp_image(noise=False)
        o.do_centroids()
        scale = o.bincube.max()
        worst["image"] = max(worst["image"], float(np.abs(cube_fused[e] - o.bincube).max() / scale),
                             float(np.abs(cube_buf[e] - o.bincube).max() / scale))
        assert np.abs(cube_buf[e] - o.bincube).max() < 2e-5 * scale
        assert np.abs(cube_fused[e] - o.bincube).max() < 2e-5 * scale
        # "bit-exact centroid indices": brightest pixel of every spot
        assert np.array_equal(cube_fused[e].argmax(axis=1), o.bincube.argmax(axis=1))
        assert np.array_equal(cube_buf[e].argmax(axis=1), o.bincube.argmax(axis=1))
        assert np.allclose(cube_fused[e].sum(axis=1), s.nphot * s.flux, rtol=1e-5)
        assert np.allclose(cube_buf[e].sum(axis=1), s.nphot * s.flux, rtol=1e-5)
        for sl in (sl_buf, sl_fused, sl_cog, sl_only):
            worst["slopes"] = max(worst["slopes"], float(np.abs(sl[e] - o.slopes).max()))
            assert np.abs(sl[e] - o.slopes).max() < 1e-4   # arcsec (north-star tolerance)
        if direct:
            assert np.abs(sl_fused[e] - o.slopes).max() < 2e-5
        if ref64:
            want = pr.slopes64(s, ph[e])
            worst["oracle64"] = max(worst["oracle64"], float(np.abs(o.slopes - want).max()))
            for sl in (sl_buf, sl_fused, sl_cog, sl_only):
                worst["slopes64"] = max(worst["slopes64"], float(np.abs(sl[e] - want).max()))
                assert np.abs(sl[e] - want).max() < 1e-4
    return worst


def check_target_psf(sim, oracles, valu, ref64=False):
    """All three PSF-row kernels: software-pipelined MFMA (0), VALU fallback (1), generic MFMA (2)."""
    s = sim.s
    sim.set_option("force_valu_target", 1 if valu == 1 else 0)
    sim.set_option("force_generic_target", 1 if valu == 2 else 0)
    push_oracle_state(sim, oracles)
    rng = np.random.default_rng(7)
    volts = rng.normal(0, 0.3, size=(len(oracles), s.nactu)).astype(np.float32)
    sim.comp_dm_shape(torch.from_numpy(volts).cuda())
    sim.reset_strehl()
    for rep in range(2):
        sim.target_psf()
        sim.comp_strehl()
    sim.raytrace_target()
    tp = sim.t["tar_phase"].cpu().numpy()
    st = sim.strehl.cpu().numpy()
    worst = dict(phase=0.0, strehl=0.0, var=0.0, strehl64=0.0, var64=0.0, oracle_sr64=0.0, oracle_var64=0.0)
    for e, o in enumerate(oracles):
        o.comp_shapes(volts[e])
        o.reset_strehl()
        o.raytrace_target()
        worst["phase"] = max(worst["phase"], float(np.abs(tp[e] - o.tar_phase).max()))
        assert np.abs(tp[e] - o.tar_phase).max() < 1e-5
        for rep in range(2):
            want = o.comp_strehl()
        worst["strehl"] = max(worst["strehl"], abs(st[e, 0] - want[0]) / max(want[0], 1e-3))
        worst["var"] = max(worst["var"], abs(st[e, 2] - want[2]) / want[2])
        assert abs(st[e, 0] - want[0]) < 2e-5 * max(want[0], 1e-3) + 1e-7
        assert abs(st[e, 1] - want[1]) < 2e-5 * max(want[1], 1e-3) + 1e-7
        assert abs(st[e, 2] - want[2]) < 1e-4 * want[2] + 1e-9
        assert abs(st[e, 3] - want[3]) < 1e-4 * want[3] + 1e-9
        # comp_strehl(do_fit=True), the reference's default: the peaks fitted by two 1-D sincs (oracle: the same
        # algorithm in double precision on its own window)
        fit, sf = o.get_strehl(do_fit=True), sim.strehl_fit.cpu().numpy()
        assert fit[0] >= want[0] and fit[1] >= want[1] and fit[0] < 1.2 * want[0] + 1e-6
        assert abs(sf[e, 0] - fit[0]) < 1e-4 * max(fit[0], 1e-3) + 1e-7, (sf[e], fit)
        assert abs(sf[e, 1] - fit[1]) < 1e-4 * max(fit[1], 1e-3) + 1e-7, (sf[e], fit)
        if ref64:
            sr64, var64 = pr.strehl64(s, tp[e]), pr.phase_var64(s, tp[e])
            worst["strehl64"] = max(worst["strehl64"], abs(st[e, 0] - sr64) / max(sr64, 1e-3))
            worst["var64"] = max(worst["var64"], abs(st[e, 2] - var64) / var64)
            worst["oracle_sr64"] = max(worst["oracle_sr64"], abs(want[0] - sr64) / max(sr64, 1e-3))
            worst["oracle_var64"] = max(worst["oracle_var64"], abs(want[2] - var64) / var64)
            assert abs(st[e, 0] - sr64) < 2e-5 * sr64 + 1e-7, (st[e, 0], sr64)
            assert abs(st[e, 1] - sr64) < 2e-5 * sr64 + 1e-7, (st[e, 1], sr64)     # two exposures of the same phase
            assert abs(st[e, 2] - var64) < 1e-4 * var64, (st[e, 2], var64)
    sim.set_option("force_valu_target", 0)
    sim.set_option("force_generic_target", 0)
    return worst


def check_fused_frame(sim, oracles, otf=True):
    """One-pass frame kernel (science PSF rows + WFS spots from the same phase tiles) vs the
    oracle and vs the separate target / WFS kernels, with and without the bincube.  otf=False: without the modes
    that evaluate the stack-array DM from the voltages.  Returns the kernel instantiation of every mode."""
    s = sim.s
    assert sim.frame_fused_available()
    push_oracle_state(sim, oracles)
    rng = np.random.default_rng(11)
    volts = rng.normal(0, 0.4, size=(len(oracles), s.nactu)).astype(np.float32)
    volts[:, -2:] = rng.normal(0, 0.05, size=(len(oracles), 2))      # tip-tilt: analytic planes
    sim.comp_dm_shape(torch.from_numpy(volts).cuda())
    out, names = {}, {}
    modes = [m for m in FRAME_MODES if otf or not m.startswith("otf")]
    for mode in modes:
        sim.reset_strehl()
        sim.set_option("force_f32_dft", 1 if mode == "otf_f32" else 0)
        if mode.startswith("otf"):
            # stack-array DM evaluated from st.voltage inside the kernel: the stored planes are
            # poisoned to prove they are not read
            assert sim.dm_from_voltage_available()
            sim.set_com(torch.from_numpy(volts).cuda())
            sim.apply_control(comp_voltage=False, defer_shape=True)
            nz = s.dms[0].dim ** 2
            sim.t["dm_shape"][:, :nz] = 1e3
            assert sim._stale
        if mode == "unfused":
            sim.target_psf()
            sim.comp_image(noise=False, write_bincube=True, cog=True)
        else:
            sim.t["bincube"].zero_()
            sim.slopes.zero_()
            sim.frame_fused(noise=False, write_bincube=mode.endswith("cube"), cog=True)
            names[mode] = sim.frame_kernel_name()
        sim.comp_strehl()
        out[mode] = (sim.slopes.cpu().numpy().copy(), sim.strehl.cpu().numpy().copy(),
                     sim.t["bincube"].cpu().numpy().copy())
    sim.set_option("force_f32_dft", -1)         # back to the library's precision mode
    # materialising afterwards restores the stored planes from the same voltages
    shp = sim.dm_shape(0).cpu().numpy()
    assert not sim._stale
    for e, o in enumerate(oracles):
        o.comp_shapes(volts[e])
        o.reset_strehl()
        o.raytrace_target()
        want = o.comp_strehl()
        o.raytrace_wfs(atm=True, dms=True, reset=True)
        o.comp_image(noise=False)
        o.do_centroids()
        assert np.abs(shp[e].ravel() - o.dm_shapes[0].ravel()).max() < 2e-6 * max(1.0, np.abs(o.dm_shapes[0]).max())
        for mode in modes[1:]:
            sl, st, cube = out[mode]
            assert np.abs(sl[e] - o.slopes).max() < 2e-5, mode
            assert np.abs(sl[e] - out["unfused"][0][e]).max() < 2e-5, mode
            assert abs(st[e, 0] - want[0]) < 2e-5 * max(want[0], 1e-3) + 1e-7, mode
            assert abs(st[e, 2] - want[2]) < 1e-4 * want[2] + 1e-9, mode
        for mode in [m for m in modes if m.endswith("cube")]:
            cube = out[mode][2]
            assert np.abs(cube[e] - o.bincube).max() < 2e-5 * o.bincube.max(), mode
            assert np.array_equal(cube[e].argmax(axis=1), o.bincube.argmax(axis=1)), mode
    return names


class _Frame(object):
    """What one oracle left behind a frame of the loop (the fields closed_loop compares)."""

    def __init__(self, o):
        self.slopes, self.com = o.slopes.copy(), o.com.copy()
        self.strehl_se, self.strehl_le = o.strehl_se, o.strehl_le


class OracleTrace(object):
    """The oracles' side of closed_loop, computed once and shared by the runs that are compared with it: the state
    behind the reset (`start`, what push_oracle_state reads), every frame of every oracle (`frames[it][e]`), and the
    OPEN-loop short-exposure Strehl ratio of the same atmosphere (flat mirrors, float64) at every frame."""

    def __init__(self, oracles, seeds, nframes=40):
        import types
        s = oracles[0].s
        for o, sd in zip(oracles, seeds):
            o.reset(sd)
        self.seeds, self.nframes = list(seeds), nframes
        self.start = [types.SimpleNamespace(screens=[scr.copy() for scr in o.screens], ext_count=list(o.ext_count),
                                            accumx=o.accumx.copy(), accumy=o.accumy.copy()) for o in oracles]
        for o in oracles:
            o.raytrace_target()
        self.frames, phases = [], []
        for it in range(nframes):
            row = []
            for o in oracles:
                o.next_part_two(None)
                o.next_part_one()
                row.append(_Frame(o))
                phases.append(gc.raytrace64(s, o.screens, [], True, dms=False))
            self.frames.append(row)
        # (behind the loop: the oracle's OpenMP regions and the BLAS threads of the float64 DFT slow each other down
        # when they alternate)
        self.open_loop = np.array([pr.strehl64(s, ph) for ph in phases]).reshape(nframes, len(oracles))


def closed_loop(sim, oracles, seeds, precision, unfused=False, defer_shape=True, nframes=40, trace=None):
    """`nframes` frames of the integrator loop (next_part_two + next_part_one) from a common pushed state against the
    oracles, frame by frame (trace: an OracleTrace of the same seeds instead of stepping `oracles`).  Returns
    (launch counts by arithmetic, worst slope deviation, the short-exposure Strehl ratios [frame, environment])."""
    from ao_marl_amd import libaomarl as la
    keep_precision = la.get_precision()
    la.set_precision(precision)
    try:
        la.arith_launches(reset=True)
        sim.set_option("force_unfused_frame", 1 if unfused else 0)
        sim.set_option("force_f32_dft", -1)
        sim.defer_shape = defer_shape
        sim.reset(seeds)
        if trace is None:
            for o, sd in zip(oracles, seeds):
                o.reset(sd)
            push_oracle_state(sim, oracles)   # remove the reset's accumulated round-off
        else:
            assert list(seeds) == trace.seeds and nframes <= trace.nframes
            push_oracle_state(sim, trace.start)
        sim.target_psf()
        if trace is None:
            for o in oracles:
                o.raytrace_target()
        worst, se = 0.0, []
        for it in range(nframes):
            sim.next_part_two(None)
            sim.next_part_one()
            sl = sim.slopes.cpu().numpy()
            cm = sim.com.cpu().numpy()
            st = sim.strehl.cpu().numpy()
            se.append(st[:, 0].copy())
            for e in range(len(seeds)):
                if trace is None:
                    o = oracles[e]
                    o.next_part_two(None)
                    o.next_part_one()
                else:
                    o = trace.frames[it][e]
                worst = max(worst, np.abs(sl[e] - o.slopes).max())
                assert np.abs(sl[e] - o.slopes).max() < 1e-4, it
                assert np.abs(cm[e] - o.com).max() < 5e-5 * np.abs(o.com).max() + 1e-3, it
                assert abs(st[e, 0] - o.strehl_se) < 1e-4, it
                assert abs(st[e, 1] - o.strehl_le) < 1e-4, it
        launched = {k: v for k, v in la.arith_launches().items() if v}
    finally:
        sim.set_option("force_unfused_frame", 0)
        sim.defer_shape = True
        la.set_precision(keep_precision)
    return launched, float(worst), np.array(se)
