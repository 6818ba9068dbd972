"""Laser guide star on the CPU: the elongation kernel against the moments of the reference's own make_lgs_prof1d
(tests/golden/lgs.npz, tools/gen_golden_lgs.py), the float64 model (ao_marl_amd/lgs.py: LgsModel) against the oracle's
Shack-Hartmann image, its two formulations against each other, flux, the cone trace, the tilt response, the refusals,
the host half of the native object under the sanitizers, and a supervisor that had a sensor attached and detached.

Bounds of the kernel test (the issue's): sigma_minor is the beam's, 1e-3 relative; sigma_major 2 % -- integrating the
profile into cells adds cell^2 / 12 to the variance, the reference uses whole pixels (0.6 % of sigma at 3.6 pixels), this
project half pixels, and the bound is three times that figure; the axis 0.5 degrees up to the sign."""
import copy
import os
import subprocess

import numpy as np
import pytest

from ao_marl_amd import geometry as G
from ao_marl_amd import lgs as L
from ao_marl_amd import params as P
from oracle import aoref
from tests import helpers
from tests import lgs_cases as lc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ao_marl_amd", "csrc")


def _oracle_image(s, phase):
    """(bincube, slopes) of the oracle's Shack-Hartmann image of one phase, noise off"""
    lib = aoref.lib()
    cube = np.zeros((s.nvalid, s.npix * s.npix), dtype=np.float32)
    lib.aoref_sh_image(np.ascontiguousarray(phase, dtype=np.float32).reshape(-1), s.mpupil.reshape(-1), s.nvalid, s.pdiam,
                       s.nfft, s.npix, s.nrebin, s.phasemap, s.halfxy.reshape(-1), s.binmap, s.flux, float(s.nphot),
                       s.wfs_lambda, cube)
    sl = np.zeros(s.nslope, dtype=np.float32)
    lib.aoref_cog(cube, s.nvalid, s.npix, s.cog_offset, s.cog_scale, sl)
    return cube, sl


# ------------------------------------------------------------------------------------------------ 1. the kernel
def test_kernel_against_the_reference_moments():
    z = lc.golden()
    ps, sysm, s = lc.system_of()
    w = sysm.wfss[0]
    assert (w.Ntot, w.Nfft, w.pdiam, w.nrebin, w.npix) == (64, 64, 16, 2, 16) == tuple(
        int(z[k]) for k in ("Ntot", "Nfft", "pdiam", "nrebin", "npix"))
    assert abs(w.qpixsize / float(z["qpixsize"]) - 1) < 1e-6 and abs(w.qpixsize - 0.1289) < 1e-4
    assert np.array_equal(w.validsubsx, z["validsubsx"]) and np.array_equal(w.validsubsy, z["validsubsy"])
    K = L.lgs_kernels(w, w, ps.p_tel, z["alt"], z["prof"], float(z["lltx"]), float(z["llty"]), float(z["beamsize"]))
    assert K.shape == (64, 64, 64) and w.nvalid == 64
    worst = np.zeros(3)
    for k in range(w.nvalid):
        major, minor, ang, _, _ = lc.moments(K[k])
        d = abs(abs(ang) - abs(z["angle"][k]))
        worst = np.maximum(worst, [abs(minor / z["sigma_minor"][k] - 1), abs(major / z["sigma_major"][k] - 1),
                                   np.degrees(min(d, np.pi - d))])
    print("worst over 64 sub-apertures: sigma_minor %.2e relative, sigma_major %.3f %%, axis %.4f degrees"
          % (worst[0], 100 * worst[1], worst[2]))
    assert worst[0] <= 1e-3 and worst[1] <= 0.02 and worst[2] <= 0.5
    # the azimuth the kernel was drawn with is the reference's own (no exchange of the axes there)
    assert np.abs(np.array([lc.moments(K[k])[2] for k in range(64)]) - z["azimuth"]).max() < np.radians(0.5)
    assert np.abs(K.sum(axis=(1, 2)) - 1).max() < 1e-12 and K.min() >= 0


def test_kernel_against_the_reference_whole_kernels():
    """Four of the reference's kernels as it stores them: first index x (transposed here), the angle's sign open (the
    better of the two mirror images), its centre half a pixel off this project's (the best whole-pixel shift of the
    circular cross-correlation).  What is left is a displacement of at most half a pixel per axis, which costs two
    Gaussians of sigma 2.635 and >= 3.56 pixels a factor exp(-0.25 / 4 sigma^2) each, 0.986 together: bound 0.98."""
    z = lc.golden()
    ps, sysm, s = lc.system_of()
    w = sysm.wfss[0]
    K = L.lgs_kernels(w, w, ps.p_tel, z["alt"], z["prof"], float(z["lltx"]), float(z["llty"]), float(z["beamsize"]))

    def peak(a, b):
        a, b = a / np.sqrt((a * a).sum()), b / np.sqrt((b * b).sum())
        c = np.fft.ifft2(np.fft.fft2(a) * np.conj(np.fft.fft2(b))).real
        iy, ix = np.unravel_index(c.argmax(), c.shape)
        return c.max(), min(iy, 64 - iy), min(ix, 64 - ix)
    for i, k in enumerate(z["whole_index"]):
        ref = z["whole"][i].astype(np.float64).T
        c, dy, dx = max(peak(K[k], ref), peak(K[k], ref[::-1]))
        print("sub-aperture %d: correlation with the reference's kernel %.4f at a shift of (%d, %d) pixels" % (k, c, dy, dx))
        assert c >= 0.98 and dy <= 1 and dx <= 1


@pytest.mark.parametrize("llt", [(0., 0.), (-3., -3.), (20., 0.)])
def test_gauss1_kernel_invariants(llt):
    K = lc.kernels(llt)
    N = K.shape[1]
    assert np.abs(K.sum(axis=(1, 2)) - 1).max() < 1e-12 and K.min() >= 0
    cen = np.array([lc.moments(k)[3:] for k in K])
    print("launch %r: centroid off (N/2, N/2) by at most %.2e pixels" % (llt, np.abs(cen - N / 2).max()))
    if max(abs(llt[0]), abs(llt[1])) < 10:           # (20 m off the spot is wider than the image: the window cuts it)
        assert np.abs(cen - N / 2).max() < 1e-6


def test_centre_launch_is_the_round_beam_on_the_axis():
    """one sub-aperture at the launch position: r = 0, the beam alone"""
    ps, sysm, s = lc.system_of()
    w = sysm.wfss[0]
    one = G.Bag(validsubsx=np.array([0]), validsubsy=np.array([0]), npix=w.npix, nxsub=1)
    alt, prof = L.lgs_profile("gauss1")
    K = L.lgs_kernels(w, one, ps.p_tel, alt, prof, 0., 0., 0.8)[0]
    major, minor, _, c0, c1 = lc.moments(K)
    sig = 0.8 / L.FWHM2SIGMA / w.qpixsize
    assert abs(major / sig - 1) < 1e-6 and abs(minor / sig - 1) < 1e-6 and abs(c0 - 32) < 1e-9 and abs(c1 - 32) < 1e-9


# ------------------------------------------------------------------------------------------------ 2. impulse kernel
def test_impulse_kernel_is_the_ngs_image():
    _, _, s = lc.system_of()
    m = L.LgsModel(s, L.impulse_kernels(s.nvalid, s.nfft), noise=-1)
    ph = lc.smooth_phases(s, 2, seed=3, waves_of_tilt=0.5).astype(np.float32)
    cube, sl = m.measure(ph)
    for e in range(2):
        oc, osl = _oracle_image(s, ph[e])
        di, ds = np.abs(cube[e] - oc).max() / oc.max(), np.abs(sl[e] - osl).max()
        print("impulse kernel against the oracle's comp_image: image %.2e of the peak, slopes %.2e arcsec" % (di, ds))
        assert di <= 1e-5 and ds <= 1e-4


# ------------------------------------------------------------------------------------------------ 3. two formulations
def test_both_formulations_agree_in_float64():
    _, _, s = lc.system_of()
    m = L.LgsModel(s, lc.kernels((-3., -3.)), noise=-1)
    for ph in lc.smooth_phases(s, 2, seed=7, waves_of_tilt=1.0):
        a, b = m.image(ph, "fft"), m.image(ph, "lags")
        ha, hb = m.hr_image(ph, "fft"), m.hr_image(ph, "lags")
        print("fft against lags: binned %.2e, whole image %.2e of the peak"
              % (np.abs(a - b).max() / a.max(), np.abs(ha - hb).max() / ha.max()))
        assert np.abs(a - b).max() <= 1e-12 * a.max() and np.abs(ha - hb).max() <= 1e-12 * ha.max()


# ------------------------------------------------------------------------------------------------ 4. flux
def test_flux_is_preserved_before_binning():
    _, _, s = lc.system_of()
    ph = lc.smooth_phases(s, 1, seed=11)[0]
    for name, llt in (("centre", (0., 0.)), ("side (20, 0) m", (20., 0.))):
        m = L.LgsModel(s, lc.kernels(llt), noise=-1)
        hr = m.hr_image(ph)
        want = m.nphot * m.flux
        assert np.abs(hr.sum(axis=(1, 2)) / want - 1).max() <= 1e-12
        lost = 1 - hr[:, m.indi:m.indi + m.w, m.indi:m.indi + m.w].sum(axis=(1, 2)) / hr.sum(axis=(1, 2))
        print("%s launch: share of the flux outside the window %.4f .. %.4f" % (name, lost.min(), lost.max()))
        # the binned image carries the Shack-Hartmann normalisation: the window's pixels sum to nphotons fluxPerSub
        assert np.abs(m.image(ph).sum(axis=1) / want - 1).max() <= 1e-12


def test_photons_follow_the_reference_rule():
    ps = lc.system_of()[0]
    w, tel, it = ps.p_wfss[0], ps.p_tel, ps.p_loop.ittime
    assert L.lgs_nphotons(w, tel, it) == pytest.approx(lc.system_of()[1].wfss[0].nphotons, rel=1e-12)
    assert L.lgs_nphotons(w, tel, it, laserpower=20., lgsreturnperwatt=22.) == pytest.approx(
        22. * 20. * w.optthroughput * (tel.diam / w.nxsub)**2 * 1e4 * it, rel=1e-12)


# ------------------------------------------------------------------------------------------------ 5. the cone
def test_cone_with_delta_one_is_the_oracle_trace():
    _, _, s = lc.system_of([0., 4500., 14000.])
    o = helpers.CalSim(s)
    rng = np.random.default_rng(5)
    for scr in o.screens:
        scr[:] = rng.normal(size=scr.shape).astype(np.float32)
    o.raytrace_wfs(atm=True, dms=False, reset=True)
    got = L.cone_trace_model(o.screens, s.wfs_atm_off, np.ones(s.nscreens), s.n, dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, o.wfs_phase)
    got64 = L.cone_trace_model(o.screens, s.wfs_atm_off, np.ones(s.nscreens), s.n)
    assert np.abs(got64 - o.wfs_phase).max() <= 1e-5 * np.abs(o.wfs_phase).max()


def test_cone_magnifies_a_ramp_about_the_pupil_centre():
    ps, sysm, s = lc.system_of([8000.])
    delta = L.cone_deltas(sysm.atm.alt, 90e3)
    assert delta.shape == (1,) and abs(delta[0] - (1 - 8000. / 90e3)) < 1e-15 and abs(delta[0] - 0.911) < 1e-3
    dim, (xo, yo) = s.screen_dim[0], s.wfs_atm_off[0]
    a, b = 0.37, -0.21
    v, u = np.indices((dim, dim)).astype(np.float64)
    out = L.cone_trace_model([a * u + b * v], s.wfs_atm_off, delta, s.n)
    c = (s.n - 1) / 2.
    yy, xx = np.indices((s.n, s.n)).astype(np.float64)
    want = a * (c + xo + delta[0] * (xx - c)) + b * (c + yo + delta[0] * (yy - c))
    assert np.abs(out - want).max() <= 1e-11 * np.abs(want).max()
    flat = L.cone_trace_model([a * u + b * v], s.wfs_atm_off, [1.0], s.n)
    ic = s.n // 2
    mid = lambda p: p[ic - 1:ic + 1, ic - 1:ic + 1].mean()  # noqa: E731  (the value at c_p, between four pixels)
    assert abs(mid(out) - mid(flat)) <= 1e-11 * abs(mid(flat))
    gx, gy = np.diff(out, axis=1), np.diff(out, axis=0)
    assert np.abs(gx - a * delta[0]).max() < 1e-10 and np.abs(gy - b * delta[0]).max() < 1e-10


# ------------------------------------------------------------------------------------------------ 6. tilt response
def _tilt_response(m, s, arcsec=0.1):
    """mean slope response (x to an x tilt, y to a y tilt) over the sub-apertures"""
    flat = m.measure(np.zeros((s.n, s.n)))[1][0]
    rx = (m.measure(lc.tilt_phase(s, arcsec, 1))[1][0] - flat)[:s.nvalid]
    ry = (m.measure(lc.tilt_phase(s, arcsec, 0))[1][0] - flat)[s.nvalid:]
    return rx, ry


def test_tilt_response():
    _, _, s = lc.system_of()
    tilt = 0.1
    m = L.LgsModel(s, lc.kernels((0., 0.)), noise=-1)
    hr = m.hr_image(np.zeros((s.n, s.n)))
    lost = float((1 - hr[:, m.indi:m.indi + m.w, m.indi:m.indi + m.w].sum(axis=(1, 2)) / hr.sum(axis=(1, 2))).max())
    rx, ry = _tilt_response(m, s, tilt)
    print("centre launch: response to %.1f arcsec of tilt x %.4f .. %.4f, y %.4f .. %.4f; window loss %.4f"
          % (tilt, rx.min(), rx.max(), ry.min(), ry.max(), lost))
    assert np.abs(np.abs(rx) / tilt - 1).max() <= lost and np.abs(np.abs(ry) / tilt - 1).max() <= lost
    ngs = L.LgsModel(s, L.impulse_kernels(s.nvalid, s.nfft), noise=-1)
    nx, _ = _tilt_response(ngs, s, tilt)
    assert np.all(np.sign(rx) == np.sign(nx))                       # the sign convention is the NGS sensor's
    # the launch 20 m off along x: the spots are elongated along x beyond the field of view
    side = L.LgsModel(s, lc.kernels((20., 0.)), noise=-1)
    sx, sy = _tilt_response(side, s, tilt)
    ratio = np.abs(sx).mean() / np.abs(sy).mean()
    print("launch 20 m off along x: response along the elongation %.4f, across it %.4f, ratio %.3f"
          % (np.abs(sx).mean() / tilt, np.abs(sy).mean() / tilt, ratio))
    assert np.all(np.abs(sx) < np.abs(sy)) and ratio < 1


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_by_name():
    ps, sysm, s = lc.system_of()
    w = sysm.wfss[0]
    alt, prof = L.lgs_profile("gauss1")
    odd = G.Bag(**dict(w.__dict__))
    odd.Ntot = 128
    with pytest.raises(NotImplementedError, match="Ntot = 128 != Nfft = 64"):
        L.lgs_kernels(odd, w, ps.p_tel, alt, prof, 0., 0., 0.8)
    with pytest.raises(ValueError, match="beamsize"):
        L.lgs_kernels(w, w, ps.p_tel, alt, prof, 0., 0., 0.)
    with pytest.raises(ValueError, match="launch telescope"):
        L.lgs_kernels(w, w, ps.p_tel, alt, prof, np.nan, 0., 0.8)
    with pytest.raises(ValueError, match="gauss1"):
        L.lgs_profile("allProfileNa_withAltitude.npy")
    with pytest.raises(ValueError, match="equally spaced"):
        L.lgs_profile((np.array([80e3, 90e3, 95e3]), np.ones(3)))
    with pytest.raises(ValueError, match="same length"):
        L.lgs_profile((np.array([80e3, 90e3]), np.ones(3)))
    with pytest.raises(ValueError, match="positive sum"):
        L.lgs_profile((np.array([80e3, 90e3]), np.zeros(2)))
    with pytest.raises(ValueError, match="not above the highest layer"):
        L.cone_deltas([0., 14000.], 14000.)
    with pytest.raises(ValueError, match="gsalt"):
        L.cone_deltas([0.], 0.)
    good = L.impulse_kernels(s.nvalid, s.nfft)
    with pytest.raises(ValueError, match="shape"):
        L.LgsModel(s, good[:3])
    bad = good.copy()
    bad[5, 0, 0] = -1e-3
    with pytest.raises(ValueError, match="not negative"):
        L.LgsModel(s, bad)
    with pytest.raises(ValueError, match="form"):
        L.LgsModel(s, good).image(np.zeros((s.n, s.n)), form="direct")
    s12 = copy.copy(s)
    s12.pdiam, s12.nfft = 12, 64
    with pytest.raises(NotImplementedError, match="pdiam = 12, N = 64: the kernel is built for pdiam = 16, N = 64, pdiam = 8"):
        L._check_size(s12)
    # what refused an LGS before still does
    ngs = P.builtin(lc.CONFIG)
    ngs.p_wfss[0].gsalt = 90e3
    with pytest.raises(NotImplementedError, match="LGS sensors are out of scope"):
        G.build_system(ngs)


def test_the_smaller_size_exists_and_the_model_runs_there():
    """geometry.sh_sizes yields a sensor with Ntot = Nfft at pdiam = 8, N = 32 (the 10x10 system on a pupil of 80
    pixels): the device kernel has that instantiation, and the model's statements hold there as well"""
    ps, sysm, s = lc.system_of(pupdiam=80)
    w = sysm.wfss[0]
    assert (w.pdiam, w.Nfft, w.Ntot, w.nrebin, w.npix) == (8, 32, 32, 2, 16) and (8, 32) in L.LGS_SIZES
    ph = lc.smooth_phases(s, 1, seed=4, rms_um=0.1)[0].astype(np.float32)
    m = L.LgsModel(s, L.impulse_kernels(s.nvalid, s.nfft), noise=-1)
    cube, sl = m.measure(ph)
    oc, osl = _oracle_image(s, ph)
    assert np.abs(cube[0] - oc).max() <= 1e-5 * oc.max() and np.abs(sl[0] - osl).max() <= 1e-4
    m = L.LgsModel(s, lc.kernels((-3., -3.), pupdiam=80), noise=-1)
    a, b = m.image(ph, "fft"), m.image(ph, "lags")
    assert np.abs(a - b).max() <= 1e-12 * a.max()


def test_host_check_builds_and_passes(tmp_path):
    """lgs_host_check.cpp under the address and undefined-behaviour sanitizers: the validators' refusals, the kernel's
    table in the lag domain against its definition, the launch plan; the Makefile's host_check target runs it too"""
    exe = str(tmp_path / "lgs_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "lgs_host_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "lgs_host_check: ok"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    line = [ln for ln in mk.splitlines() if "_host_check.cpp" in ln][0]
    assert " lgs " in line and "aomarl_lgs.hip" in mk and "aomarl_lgs_host.h" in mk


# ------------------------------------------------------------------------------------------------ 8. nothing attached
def _run(sup, frames=3):
    sup.reset()
    sup.next_part_one()
    out = []
    for _ in range(frames):
        sup.next_part_two(None, linear_control=True)
        sup.next_part_one()
        out.append(np.concatenate([np.asarray(sup.get_slopes()).ravel(), np.asarray(sup.get_command()).ravel(),
                                   np.asarray(sup.get_err()).ravel(), np.asarray(sup.get_strehl()).ravel()]))
    return np.stack(out)


def test_a_detached_sensor_leaves_the_supervisor_as_it_was():
    from ao_marl_amd.env import VecRlSupervisor
    from tests.oracle_vecsim import OracleVecSim
    kw = dict(device="cpu", sim_factory=OracleVecSim)
    plain = VecRlSupervisor(lc.CONFIG, dict(n_reverse_filtered_from_cmat=5), 2, **kw)
    sup = VecRlSupervisor(lc.CONFIG, dict(n_reverse_filtered_from_cmat=5), 2, **kw)
    assert sup.lgs is None
    sen = L.LgsSensor(sup, gsalt=90e3, llt=(-3., -3.))
    assert sen.kernels.shape == (64, 64, 64) and sen.nphotons == pytest.approx(float(sup.s.nphot), rel=1e-6)
    with pytest.raises(RuntimeError, match="calibrate"):
        sen.start()
    cmat = sen.calibrate()
    print("CPU calibration: doubled-push deviation %.3g" % sen.linearity)
    assert cmat.shape == (sup.s.nactu, sup.s.nslope) and sen.linearity < 0.05
    sen.start()
    assert sup.lgs is sen and sup.get_slopes() is sen.slopes
    sen2 = L.LgsSensor(sup, kernels=L.impulse_kernels(64, 64))
    sen2.cmat = cmat
    with pytest.raises(RuntimeError, match="LGS attached already"):
        sen2.start()
    with pytest.raises(RuntimeError, match="stop"):
        sen.calibrate()
    sen.stop()
    sen.stop()
    assert sup.lgs is None
    a, b = _run(plain), _run(sup)
    assert a.shape == b.shape and np.array_equal(a, b)
    # the refusals of start(): the supervisor states the pyramid refuses, plus an attached pyramid or registration
    for attr, val, match in (("pyramid", object(), "pyramid is attached"), ("registration", object(), "mis-registration"),
                             ("pure_delay_0", True, "pure-delay-0"), ("autoencoder", object(), "denoiser"),
                             ("geo", object(), "GEO twin"),
                             ("online_modal_gains", object(), "on-line modal-gain"),
                             ("modal_predictor", object(), "modal predictor"), ("reset_prefetch", object(), "prefetched reset"),
                             ("gain", None, "per-environment gains")):
        old = getattr(sup, attr, None)
        setattr(sup, attr, val)
        try:
            with pytest.raises((RuntimeError, NotImplementedError), match=match):
                sen.start()
        finally:
            setattr(sup, attr, old)
    sup.sim.get_modal_gains = lambda: np.ones((1, 3))           # (the supervisor reads its modal gains from the simulator)
    with pytest.raises(RuntimeError, match="modal gains are set"):
        sen.start()
    del sup.sim.get_modal_gains
    assert sup.lgs is None
    with pytest.raises(ValueError, match="gsalt = 0.0 m must be positive"):
        L.LgsSensor(sup, gsalt=0.)
    # a seen mirror above the ground would be seen through the cone: refused by name
    keep_alt, sup.s.dms[0].alt = sup.s.dms[0].alt, 1000.
    try:
        with pytest.raises(NotImplementedError, match="conjugated to 1000 m"):
            L.LgsSensor(sup)
    finally:
        sup.s.dms[0].alt = keep_alt
    # the loop on the CPU: with the impulse kernel, the guide star at 1e9 m and the supervisor's own command matrix it
    # is the Shack-Hartmann loop (float64 model against the oracle's float32 image: the project's parity figures)
    ngs = L.LgsSensor(sup, gsalt=1e9, kernels=L.impulse_kernels(64, 64), noise=-1)
    ngs.cmat = np.asarray(sup.s.cmat)
    ngs.start()
    try:
        c = _run(sup, frames=2)
    finally:
        ngs.stop()
    ns, na = sup.s.nslope * 2, sup.s.nactu * 2
    d_sl, d_com = np.abs(c[:, :ns] - a[:2, :ns]).max(), np.abs(c[:, ns:ns + na] - a[:2, ns:ns + na]).max()
    print("CPU loop, impulse kernel against the SH loop: slopes %.2e arcsec, commands %.2e of %.2f"
          % (d_sl, d_com, np.abs(a[:2, ns:ns + na]).max()))
    assert d_sl <= 1e-4 and d_com <= 2e-4 * np.abs(a[:2, ns:ns + na]).max() + 5e-3
