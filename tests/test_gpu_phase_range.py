"""Every frame kernel at phases far past the +-256 revolutions of v_sin_f32 / v_cos_f32 (128 um at the sensor's 0.5 um,
422 um at the science 1.65 um), against the same frame without the offset and against float64 references.

Offsets Delta = P K (tests/phase_range.py: P = 16.5 um, a whole number of both wavelengths) change no slope, no spot and
no Strehl ratio: A, a whole-layer piston of +-33 P (only the science argument of the paths that do not subtract the
phase at the pupil centre sees it); B, random K in [-40, 40] per 5 x 5 pixels (steps inside every sub-aperture), K = 0
at the pupil centre, so that |phase - phase at the centre| reaches 660 um in every path.  C drives the mirrors to
about 300 um of stroke: slopes against the float64 centre of gravity of the raytraced phase and against the oracle.
Frames here never move the screens (an extrusion would turn P K into non-multiples of P on its new lines)."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ao_marl_amd import geometry as G, params, system  # noqa: E402
from oracle import aoref  # noqa: E402
from tests import helpers, phase_range as pr  # noqa: E402

NAME = "production_sh_10x10_2m"
L_NAME = "production_sh_40x40_8m_3layers"
SEEDS = [1234, 1250]
STROKE = 300.0                  # um of mirror stroke (max |phase - phase at the centre|) in case C
# Case C slopes (arcsec) against the float64 centre of gravity of the raytraced phase and against the oracle.  Half an
# ulp of 300 um is 3e-5 sensor waves per pixel: the oracle's own fp32 arguments put it 8e-5 off the float64 slopes,
# and the stack-array DM evaluated on the matrix cores (the OTF instantiations) rounds differently from the stored
# shape the references trace (measured on the MI355X: 3e-5 for the kernels that read the stored shape, 7.8e-5 for the
# OTF split-fp16 ones, 1.06e-4 for the slopes-only fp32 one).
TOL_C = 1.5e-4

# 10x10: the six modes of test_gpu_parity.py::test_fused_frame_matches_oracle_and_unfused ("unfused" = generic spot 0 +
# PSF rows 0), the generic spot kernel and the two other PSF-row kernels (these reduce their arguments: controls).
# name: (how, force_generic_spot, PSF-row kernel, force_f32_dft, write_bincube, expected instantiation or None)
SMALL_MODES = {
    "unfused": ("sep", 0, 0, -1, True, None),
    "generic_spot": ("sep", 1, 0, -1, True, None),
    "valu1": ("sep", 0, 1, -1, True, None),
    "valu2": ("sep", 0, 2, -1, True, None),
    "fused_cube": ("shape", 0, 0, 0, True, (False, True, True)),
    "fused": ("shape", 0, 0, 0, False, (False, False, True)),
    "otf_cube": ("otf", 0, 0, 0, True, (True, True, True)),
    "otf": ("otf", 0, 0, 0, False, (True, False, True)),
    "otf_f32": ("otf", 0, 0, 1, False, (True, False, False)),
}
# 40x40: every entry of tests/test_gpu_large.py::LARGE_CASES, (unfused, write_bincube, precision)
LARGE_MODES = {"%d_%s_%s" % c: c for c in [(0, True, "f32"), (1, True, "f32"), (2, True, "f32"), (0, False, "f32"),
                                           (0, False, "split_f16"), (0, True, "split_f16")]}
NAME_RE = re.compile(r"k_frame_wave<\d+, \d+, (true|false), false, (true|false), (true|false)>")


def _smooth_screens(s, nenv, rng):
    out = []
    for d in s.screen_dim:
        f = rng.normal(size=(nenv, d // 8 + 2, d // 8 + 2))
        up = np.kron(f, np.ones((8, 8)))[:, :d, :d]
        k = np.ones(15) / 15.0
        for ax in (1, 2):
            up = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, up)
        out.append((4.0 * up).astype(np.float32))
    return out


def _cases(s, base, rng):
    """Screens per case: none, A (piston +-33 P on layer 0), B (integer-period blocks on layer 0), neg (B plus a
    quarter sensor wave on alternate 5-pixel blocks: must move the results)."""
    P = pr.common_period(s)
    d = s.screen_dim[0]
    nenv = base[0].shape[0]
    ctr = pr.pupil_centre_on_layer(s, 0)
    dA = np.stack([pr.offset_field(P, pr.piston_field(d, 33 * (1 - 2 * (e % 2)))) for e in range(nenv)])
    dB = np.stack([pr.offset_field(P, pr.block_field(d, rng, centre=ctr, clear=3)) for e in range(nenv)])
    yy, xx = np.mgrid[0:d, 0:d]
    quarter = np.float32(0.25 * float(s.wfs_lambda)) * (((yy // 5) + (xx // 5)) % 2).astype(np.float32)
    deltas = {"none": np.zeros_like(dA), "A": dA, "B": dB, "neg": dB + quarter}
    return {k: [base[0] + v] + list(base[1:]) for k, v in deltas.items()}, deltas


def _sep_frame(sim, spot, rows):
    sim.set_option("force_generic_spot", spot)
    sim.set_option("force_valu_target", 1 if rows == 1 else 0)
    sim.set_option("force_generic_target", 1 if rows == 2 else 0)
    try:
        sim.target_psf()
        sim.comp_image(noise=False, write_bincube=True, cog=True)
    finally:
        for k in ("force_generic_spot", "force_valu_target", "force_generic_target"):
            sim.set_option(k, 0)


def _frame_small(sim, mode, volts):
    how, spot, rows, dft, cube, want = SMALL_MODES[mode]
    vt = torch.from_numpy(volts).cuda()
    if how == "otf":
        sim.set_com(vt)
        sim.apply_control(comp_voltage=False, defer_shape=True)
        assert sim._stale
    else:
        sim.comp_dm_shape(vt)
    sim.reset_strehl()
    if how == "sep":
        _sep_frame(sim, spot, rows)
    else:
        sim.set_option("force_f32_dft", dft)
        try:
            sim.frame_fused(noise=False, write_bincube=cube, cog=True)
        finally:
            sim.set_option("force_f32_dft", -1)
        m = NAME_RE.fullmatch(sim.frame_kernel_name())
        assert m and tuple(g == "true" for g in m.groups()) == want, (mode, sim.frame_kernel_name())
    sim.comp_strehl()
    return cube


def _frame_large(sim, mode, volts):
    from ao_marl_amd import libaomarl as la
    unfused, cube, precision = LARGE_MODES[mode]
    keep = la.get_precision()
    la.set_precision(precision)
    try:
        vt = torch.from_numpy(volts).cuda()
        sim.set_option("force_unfused_frame", 1 if unfused == 1 else 0)
        if unfused == 0:
            sim.set_com(vt)
            sim.apply_control(comp_voltage=False, defer_shape=True)
        else:
            sim.comp_dm_shape(vt)
        sim.reset_strehl()
        if unfused == 1:
            sim.target_psf()
            sim.comp_image(noise=False, write_bincube=cube, cog=True)
        else:
            sim.frame_fused(noise=False, write_bincube=cube, cog=True)
            want = "k_frame_wave<3, 1, %s, false, %s, %s>" % ("true" if unfused == 0 else "false",
                                                              "true" if cube else "false",
                                                              "true" if precision == "split_f16" else "false")
            assert sim.frame_kernel_name() == want, (mode, sim.frame_kernel_name())
        sim.comp_strehl()
    finally:
        sim.set_option("force_unfused_frame", 0)
        la.set_precision(keep)
    return cube


def _outputs(sim, cube):
    return (sim.slopes.cpu().numpy().astype(np.float64), sim.strehl.cpu().numpy().astype(np.float64),
            sim.t["bincube"].cpu().numpy().astype(np.float64) if cube else None)


def _readback(sim, s, screens, volts):
    """What the kernels receive: the raytraced sensor and target phases of these screens and commands."""
    for l, scr in enumerate(screens):
        sim.set_screen(l, scr)
    sim.comp_dm_shape(torch.from_numpy(volts).cuda())
    sim.raytrace_wfs(atm=True, dms=True, reset=True)
    sim.raytrace_target(atm=True, dms=True, reset=True)
    return sim.t["wfs_phase"].cpu().numpy().copy(), sim.t["tar_phase"].cpu().numpy().copy()


def _traced(s, delta, off, n):
    """A layer offset traced to a pupil grid (integer offsets: bilinear weights 0, the values themselves)."""
    ox, oy = int(off[0]), int(off[1])
    assert float(off[0]) == ox and float(off[1]) == oy
    return delta[:, oy:oy + n, ox:ox + n].astype(np.float64)


def _check(s, sim, frame, modes, base, volts, volts_c, oracle_c, subaps, rng):
    nenv = base[0].shape[0]
    screens, deltas = _cases(s, base, rng)
    fails, table = [], []

    def want(ok, what):
        if not ok:
            fails.append(what)

    # ---- what the kernels receive: phase + Delta, and float64 references of it
    ref = {}
    for case, scr in screens.items():
        wfs, tar = _readback(sim, s, scr, volts)
        ref[case] = dict(wfs=wfs, tar=tar)
    for case in ("A", "B", "neg"):
        for key, off, n in (("wfs", s.wfs_atm_off[0], s.n), ("tar", s.tar_atm_off[0], s.pupdiam)):
            dt = _traced(s, deltas[case], off, n)
            got = ref[case][key].astype(np.float64) - ref["none"][key].astype(np.float64)
            big = float(np.abs(ref[case][key]).max())
            # fp32 sums of the layers and mirrors at the size of phase + Delta: half an ulp per term
            nterm = s.nscreens + len(s.dms) + 1
            want(np.abs(got - dt).max() <= 0.5 * nterm * np.spacing(np.float32(big)), ("raytrace", case, key))
        if case != "neg":
            maxabs = float(np.abs(ref[case]["tar"]).max())
            assert maxabs > 1.2 * 256 * float(s.tar_lambda), (case, maxabs)     # past the science limit
    for case in ("none", "A", "B"):
        r = ref[case]
        r["sl64"] = np.stack([pr.slopes64(s, r["wfs"][e], subaps) for e in range(nenv)])
        r["sr64"] = np.array([pr.strehl64(s, r["tar"][e]) for e in range(nenv)])
        r["var64"] = np.array([pr.phase_var64(s, r["tar"][e]) for e in range(nenv)])
        if case != "none":
            # the float64 truth of the phase the kernels receive, Delta taken off exactly: what the fp32 rounding of
            # phase + Delta alone moves the results by (a wrong period would NOT show here)
            back_w = ref[case]["wfs"].astype(np.float64) - _traced(s, deltas[case], s.wfs_atm_off[0], s.n)
            back_t = ref[case]["tar"].astype(np.float64) - _traced(s, deltas[case], s.tar_atm_off[0], s.pupdiam)
            sl_b = np.stack([pr.slopes64(s, back_w[e], subaps) for e in range(nenv)])
            sr_b = np.array([pr.strehl64(s, back_t[e]) for e in range(nenv)])
            r["dsl_round"] = float(np.nanmax(np.abs(sl_b - ref["none"]["sl64"])))
            r["dsr_round"] = np.abs(sr_b - ref["none"]["sr64"])
            r["eps"] = 2 * np.pi * float(np.spacing(np.float32(np.abs(r["wfs"]).max()))) / float(s.wfs_lambda)
    sel = np.r_[subaps, s.nvalid + subaps]

    for mode in modes:
        out = {}
        for case, scr in screens.items():
            for l, sc in enumerate(scr):
                sim.set_screen(l, sc)
            cube = frame(sim, mode, volts)
            out[case] = _outputs(sim, cube)
        sl0, st0, cb0 = out["none"]
        for case in ("A", "B"):
            sl, st, cb = out[case]
            r = ref[case]
            tol_sl = 2e-5 + 3.0 * r["dsl_round"]
            d_sl = float(np.abs(sl - sl0).max())
            d_64 = float(np.nanmax(np.abs(sl[:, sel] - r["sl64"][:, sel])))
            tol_sr = 2e-5 * np.maximum(st0[:, 0], 1e-3) + 1e-7 + 3.0 * r["dsr_round"]
            d_se = np.abs(st[:, 0] - st0[:, 0])
            d_le = np.abs(st[:, 1] - st0[:, 1])
            d_var = np.abs(st[:, 2] - r["var64"]) / r["var64"]
            want(d_sl < tol_sl, (mode, case, "slopes vs no offset", d_sl, tol_sl))
            want(d_64 < 1e-4 + 3.0 * r["dsl_round"], (mode, case, "slopes vs float64", d_64))
            want((d_se < tol_sr).all(), (mode, case, "SE Strehl", d_se, tol_sr))
            want((d_le < tol_sr).all(), (mode, case, "LE Strehl", d_le, tol_sr))
            want((d_var < 1e-4).all(), (mode, case, "phase variance vs float64", d_var))
            row = [mode, case, d_sl, float((d_se / np.maximum(st0[:, 0], 1e-3)).max()), float(d_var.max())]
            if cb is not None:
                # a pixel of a spot moves by about 2 eps of the peak for eps of phase error per pupil pixel
                tol_im = (2e-5 + 2.0 * r["eps"]) * cb0.max(axis=2, keepdims=True)
                d_im = np.abs(cb - cb0)
                want((d_im <= tol_im).all(), (mode, case, "image", float((d_im / tol_im).max())))
                top2 = np.sort(cb0, axis=2)[:, :, -2:]
                clear = (top2[..., 1] - top2[..., 0]) > 4.0 * tol_im[..., 0]
                want(np.array_equal(cb.argmax(axis=2)[clear], cb0.argmax(axis=2)[clear]), (mode, case, "brightest"))
                row.append(float((d_im / cb0.max(axis=2, keepdims=True)).max()))
            table.append(row)
        # negative control: a quarter sensor wave on alternate blocks moves slopes and Strehl far past the tolerances
        sl, st, _ = out["neg"]
        tol_sr = 2e-5 * np.maximum(st0[:, 0], 1e-3) + 1e-7 + 3.0 * ref["B"]["dsr_round"]
        want(np.abs(sl - sl0).max() > 10 * (2e-5 + 3.0 * ref["B"]["dsl_round"]), (mode, "neg", "slopes did not move"))
        want((np.abs(st[:, 0] - st0[:, 0]) > 10 * tol_sr).all(), (mode, "neg", "SE Strehl did not move"))

    # ---- C: large mirror stroke
    wfs_c, tar_c = _readback(sim, s, screens["none"], volts_c)
    sl64_c = np.stack([pr.slopes64(s, wfs_c[e], subaps) for e in range(nenv)])
    var64_c = np.array([pr.phase_var64(s, tar_c[e]) for e in range(nenv)])
    mask = np.asarray(s.mpupil) > 0
    stroke = max(float(np.abs(wfs_c[e][mask] - wfs_c[e][s.n // 2, s.n // 2]).max()) for e in range(nenv))
    assert 0.7 * STROKE < stroke < 1.5 * STROKE, stroke
    for e, o in enumerate(oracle_c):
        want(np.abs(wfs_c[e] - o.wfs_phase).max() < 4e-6 * stroke, ("C", "raytrace vs oracle", e))
    for mode in modes:
        for l, sc in enumerate(screens["none"]):
            sim.set_screen(l, sc)
        frame(sim, mode, volts_c)
        sl, st, _ = _outputs(sim, False)
        d_64 = float(np.nanmax(np.abs(sl[:, sel] - sl64_c[:, sel])))
        d_or = float(max(np.abs(sl[e] - o.slopes).max() for e, o in enumerate(oracle_c)))
        d_var = np.abs(st[:, 2] - var64_c) / var64_c
        want(d_64 < TOL_C, (mode, "C", "slopes vs float64", d_64))
        want(d_or < TOL_C, (mode, "C", "slopes vs oracle", d_or))
        want((d_var < 1e-4).all(), (mode, "C", "phase variance vs float64", d_var))
        table.append([mode, "C", d_64, d_or, float(d_var.max())])
    print("\nmode case |dslope| arcsec, |dSR|/SR (C: vs oracle), |dvar|/var, |dimg|/max")
    for row in table:
        print(" ".join(str(x) if isinstance(x, str) else "%.3g" % x for x in row))
    assert not fails, "\n".join(str(f) for f in fails)


def _stroke_volts(s, o, rng, nenv):
    """Commands (pzt voltages and tip-tilt together) scaled to about STROKE um of max |phase - phase at the centre|
    over the sensor pupil."""
    mask = np.asarray(s.mpupil) > 0
    out = []
    for _ in range(nenv):
        v = rng.normal(0, 1.0, size=s.nactu).astype(np.float32)
        o.comp_shapes(v)
        o.raytrace_wfs(atm=False, dms=True, reset=True)
        ph = o.wfs_phase
        out.append((v * np.float32(STROKE / np.abs(ph[mask] - ph[s.n // 2, s.n // 2]).max())).astype(np.float32))
    return np.stack(out)


def _oracle_c(o_cls, s, base, volts_c):
    res = []
    for e in range(volts_c.shape[0]):
        o = o_cls(s, seed=SEEDS[e])
        for l in range(s.nscreens):
            o.screens[l][:] = base[l][e]
        o.comp_shapes(volts_c[e])
        o.raytrace_wfs(atm=True, dms=True, reset=True)
        o.comp_image(noise=False)
        o.do_centroids()
        res.append(o)
    return res


def test_small_frames_at_large_phase():
    from ao_marl_amd.sim import HipSim
    _, s, _ = helpers.calibrated(NAME)
    sim = HipSim(s, nenv=len(SEEDS), keep_bincube=True, keep_phase=True)
    assert sim.frame_fused_available() and sim.dm_from_voltage_available()
    sim.reset(SEEDS)
    oracles = [aoref.OracleSim(s, seed=sd) for sd in SEEDS]
    base = [np.stack([o.screens[l] for o in oracles]) for l in range(s.nscreens)]
    rng = np.random.default_rng(11)
    volts = rng.normal(0, 0.4, size=(len(SEEDS), s.nactu)).astype(np.float32)
    volts[:, -2:] = rng.normal(0, 0.05, size=(len(SEEDS), 2))
    volts_c = _stroke_volts(s, oracles[0], rng, len(SEEDS))
    oracle_c = _oracle_c(aoref.OracleSim, s, base, volts_c)
    _check(s, sim, _frame_small, list(SMALL_MODES), base, volts, volts_c, oracle_c, np.arange(s.nvalid), rng)


def test_large_frames_at_large_phase():
    from ao_marl_amd.sim import HipSim
    sysm = G.build_system(params.builtin(L_NAME))
    s = system.from_system(sysm, strehl_halfwin=8)
    s.cmat = np.zeros((s.nactu, s.nslope), dtype=np.float32)      # these frames never run the controller
    sim = HipSim(s, nenv=len(SEEDS), keep_bincube=True, keep_phase=True)
    assert sim.frame_fused_available() and sim.dm_from_voltage_available()
    rng = np.random.default_rng(12)
    base = _smooth_screens(s, len(SEEDS), rng)
    volts = (rng.normal(0, 0.3, size=(len(SEEDS), s.nactu))).astype(np.float32)
    o = helpers.QuickOracle(s, seed=SEEDS[0])
    volts_c = _stroke_volts(s, o, rng, len(SEEDS))
    oracle_c = _oracle_c(helpers.QuickOracle, s, base, volts_c)
    _check(s, sim, _frame_large, list(LARGE_MODES), base, volts, volts_c, oracle_c, pr.subap_sample(s, 200), rng)
