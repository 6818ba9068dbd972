#!/usr/bin/env python3
"""The reference's OWN GROOT functions (guardians/groot.py compute_Cerr_cpu, compute_Calias, compute_dCmm, compute_Ca_cpu,
compute_Cn_cpu, compute_OTF_fitting; guardians/starlord.py; shesha/ao/tomo.py create_nact_geom), unmodified, on two small
synthetic ROKET files -> tests/golden/groot.npz: the inputs (the file's datasets and attributes) and the reference's
outputs.

Build container only (needs the reference tree).  The file is a dict-backed stand-in for h5py.File; groot.py imports
h5py, a carmaWrap context and sutraWrap's Groot at module level, which get stand-ins here (Groot raises: only the CPU
functions run).

    case  actuators         sub-apertures  layers  L0 [m]         wind [m/s]     guide star ["]   pupil
    A     45 (7 x 7 clipped)  24 (7 x 7)     2       25, 1e5        10, 20         on axis          1.5 m, 48 px, cobs 0.2
    B     69 (9 x 9 clipped)  44 (8 x 8)     3       2, 1e5, 25     0.4, 20, 15    (5, -3)          2 m, 56 px
Case B reaches both branches of rodconan and both of Ij0t83 (the generator counts them and refuses otherwise).
create_nact_geom also runs on the kept actuators of the 10x10 and 40x40 production systems (kept: modal.correct_dm on the
geometric interaction matrix of the CPU oracle); the 40x40 matrix is stored as CSR.

Usage: python tools/gen_golden_groot.py
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
os.environ.setdefault("MPLBACKEND", "Agg")
import gen_golden_psf_rec as gp  # noqa: E402

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

CASES = {
    "A": dict(nact=7, clip=3.7, pupdiam=48, diam=1.5, cobs=0.2, nssp=7, nsub=24, seed=21,
              atmos=dict(r0=0.16, alt=[0., 6000.], L0=[25., 1e5], windspeed=[10., 20.], winddir=[0., 40.], frac=[0.7, 0.3]),
              wfs=dict(xpos=0., ypos=0., noise=3.0, gsmag=9.0), gain=0.4),
    "B": dict(nact=9, clip=4.6, pupdiam=56, diam=2.0, cobs=0.0, nssp=8, nsub=44, seed=22,
              atmos=dict(r0=0.12, alt=[0., 4000., 10000.], L0=[2., 1e5, 25.], windspeed=[0.4, 20., 15.],
                         winddir=[10., -75., 200.], frac=[0.5, 0.3, 0.2]),
              wfs=dict(xpos=5., ypos=-3., noise=1.0, gsmag=11.0), gain=0.4),
}
# separations that straddle every branch for x0 = 0.25 m and these outer scales
R_VECTOR = np.array([0., 1e-6, 1e-3, 0.0039, 0.00397, 0.004, 0.01, 0.1, 0.25, 1., 1.49, 1.5, 1.51, 2.9, 3.0, 7.4, 7.5, 7.6, 18.7,
                     18.8, 30., 100., 1747., 1753., 2000., 1e4, 7.4e4, 7.6e4, 2e5, 1e6])
L0_VECTOR = (2., 25., 1e5)


def install_stand_ins():
    gp.install_stand_ins()
    gp.FILES.clear()

    class Groot(object):
        def __init__(self, *a, **k):
            raise RuntimeError("COMPASS's Groot is not available: only the CPU functions run here")

    sys.modules["sutraWrap"].Groot = Groot


def make_case(nact, clip, pupdiam, diam, cobs, nssp, nsub, seed, atmos, wfs, gain):
    rng = np.random.default_rng(seed)
    pitch = pupdiam // (nact - 1)
    assert pitch * (nact - 1) == pupdiam
    pupshape = int(2 ** np.ceil(np.log2(pupdiam) + 1))
    g = np.arange(nact) - (nact - 1) / 2.0
    gx, gy = np.tile(g, nact), np.repeat(g, nact)                       # x runs fastest, as in the product's mirrors
    sel = np.hypot(gx, gy) <= clip
    gx, gy = gx[sel], gy[sel]
    na = gx.size
    xpos, ypos = gx * pitch + pupshape / 2, gy * pitch + pupshape / 2
    # the support create_nact_geom works on: two pitches of margin, corner pixels like p_dm._i1 / _j1
    dim = pupdiam + 4 * pitch + 1
    i1 = (gx * pitch + dim // 2).astype(np.int32)
    j1 = (gy * pitch + dim // 2).astype(np.int32)
    p_dm = types.SimpleNamespace(_ntotact=na, coupling=0.2, _n1=1, _n2=dim, _i1=i1, _j1=j1, _pitch=float(pitch))
    from shesha.ao.tomo import create_nact_geom
    # its float32 values in a float64 array: np.linalg.inv of a float32 matrix is a float32 inverse (:200-201), which
    # would pin every output to 1e-7 only; the product inverts in float64 whatever the file's type
    Nact = create_nact_geom(p_dm).astype(np.float64)
    # pupil, influence functions, tip and tilt
    p = pupdiam
    y, x = np.mgrid[:p, :p] - (p - 1) / 2.0
    r = np.hypot(x, y) / (p / 2.0)
    spup = ((r <= 1.0) & (r >= cobs)).astype(np.float32)
    lit = np.nonzero(spup)
    d2 = (y[lit][None, :] - gy[:, None] * pitch) ** 2 + (x[lit][None, :] - gx[:, None] * pitch) ** 2
    infl = np.exp(-d2 / (0.7 * pitch) ** 2) * (d2 <= (2.2 * pitch) ** 2)
    IF = sp.csr_matrix(infl.astype(np.float32))
    TT = np.stack([x[lit], y[lit]], axis=1).astype(np.float32) / (p / 2.0)
    nactu, nmodes = na + 2, na - 1
    Q, _ = np.linalg.qr(rng.normal(size=(nactu, nmodes)))
    Btt = Q * rng.uniform(0.5, 1.5, size=nmodes)
    P = np.linalg.pinv(Btt)
    R = rng.normal(size=(nactu, 2 * nsub)) * 0.05
    data = {"spup": spup, "IF.data": IF.data, "IF.indices": IF.indices, "IF.indptr": IF.indptr, "TT": TT, "P": P, "Btt": Btt,
            "R": R, "Nact": Nact, "dm.xpos": xpos, "dm.ypos": ypos}
    frac = np.asarray(atmos["frac"], dtype=np.float64)
    attrs = {"_Param_target__Lambda": np.array([1.65]), "_Param_atmos__r0": atmos["r0"],
             "_Param_atmos__alt": np.asarray(atmos["alt"]), "_Param_atmos__L0": np.asarray(atmos["L0"]),
             "_Param_atmos__windspeed": np.asarray(atmos["windspeed"]), "_Param_atmos__winddir": np.asarray(atmos["winddir"]),
             "_Param_atmos__frac": frac / frac.sum(), "_Param_atmos__nscreens": int(frac.size), "_Param_loop__ittime": 0.002,
             "_Param_controller__gain": gain, "_Param_wfs__xpos": np.array([wfs["xpos"]]),
             "_Param_wfs__ypos": np.array([wfs["ypos"]]), "_Param_wfs__Lambda": np.array([0.5]),
             "_Param_wfs__nxsub": np.array([nssp]), "_Param_wfs__npix": np.array([6]),
             "_Param_wfs__noise": np.array([wfs["noise"]]), "_Param_wfs__zerop": np.array([1e11]),
             "_Param_wfs__gsmag": np.array([wfs["gsmag"]]), "_Param_wfs__optthroughput": np.array([0.5]),
             "_Param_wfs__pixsize": np.array([0.3]), "_Param_tel__diam": diam, "_Param_tel__cobs": cobs,
             "_Param_geom__pupdiam": pupdiam, "_Param_dm__nact": np.array([nact, 2])}
    assert na == {7: 45, 9: 69}[nact], na
    return dict(data=data, attrs=attrs), dict(i1=i1, j1=j1, pitch=pitch, dim=dim)


def count_branches(starlord):
    """wrap the reference's Ij0t83 and rodconan so that they count the evaluations per branch"""
    counts = {"ij0_series": 0, "ij0_table": 0, "rodconan_series": 0, "rodconan_asymptotic": 0}
    ij0, rod = starlord.Ij0t83, starlord.rodconan

    def Ij0t83(x, tabx, taby):
        small = int((x < np.exp(-3.0)).sum())
        counts["ij0_series"] += small
        counts["ij0_table"] += int(x.size) - small
        return ij0(x, tabx, taby)

    def rodconan(r, L0):
        large = int(((2 * np.pi / L0) * r > 4.71239).sum())
        counts["rodconan_asymptotic"] += large
        counts["rodconan_series"] += int(np.size(r)) - large
        return rod(r, L0)

    starlord.Ij0t83, starlord.rodconan = Ij0t83, rodconan
    return counts


def kept_actuators(name):
    """(i1, j1, pitch, dim, coupling) of the stack array of a production system behind modal.correct_dm"""
    from tests import helpers
    from ao_marl_amd import modal, params
    sysm, s = helpers.uncalibrated(name)
    be = helpers.OracleBackend(s)
    modal.correct_dm(s, sysm, modal.imat_geom(s, be), be)
    dm = s.dms[0]
    return dm.i1, dm.j1, float(dm.pitch), int(dm.n2 - dm.n1 + 1), float(params.builtin(name).p_dms[s.dm_index[0]].coupling)


def main():
    install_stand_ins()
    from guardians import groot, starlord
    from shesha.ao.tomo import create_nact_geom
    counts = count_branches(starlord)
    out = {}
    for name, c in sorted(CASES.items()):
        gp.FILES[name], lattice = make_case(**c)
        f = gp.FILES[name]
        for k in counts:
            counts[k] = 0
        res = {"cerr_modal": groot.compute_Cerr_cpu(name, modal=True), "cerr_actu": groot.compute_Cerr_cpu(name, modal=False),
               "calias_slopes_3": groot.compute_Calias(name, slopes_space=True, npts=3),
               "calias_slopes_5": groot.compute_Calias(name, slopes_space=True, npts=5),
               "calias_modal_3": groot.compute_Calias(name, npts=3), "dcmm": groot.compute_dCmm(name),
               "dcmm_dk2": groot.compute_dCmm(name, ws=np.asarray(c["atmos"]["windspeed"]) * 0.5,
                                              wd=np.asarray(c["atmos"]["winddir"]) + 30., dk=2),
               "ca_gendron": groot.compute_Ca_cpu(name), "cn_model": groot.compute_Cn_cpu(name, model="model")}
        print("case %s: %d actuators, %d sub-apertures, branches %r" % (name, f["data"]["dm.xpos"].size, c["nsub"], counts))
        if name == "B":
            assert all(v > 0 for v in counts.values()), counts
            for k, v in counts.items():
                out["B_count_" + k] = np.asarray(v)
        from ao_marl_amd import psf_rec
        otftel = psf_rec.telescope_otf(f["data"]["spup"])["otftel"]
        res["otf_fit"], res["psf_fit"] = groot.compute_OTF_fitting(name, otftel)
        res["psf_fit"] = res["psf_fit"].astype(np.float64)
        for k, v in res.items():
            assert np.all(np.isfinite(v)), (name, k)
            out["%s_out_%s" % (name, k)] = np.asarray(v, dtype=np.float64)
        for k, v in f["data"].items():
            out["%s_%s" % (name, k)] = v
        for k, v in f["attrs"].items():
            out["%s_%s" % (name, k)] = np.asarray(v)
        out["%s_tar_lambda" % name] = np.array([1.65])
        for k, v in lattice.items():
            out["%s_lattice_%s" % (name, k)] = np.asarray(v)
    # the structure functions
    tabx, taby = starlord.tabulateIj0()
    out["fn_r"] = R_VECTOR
    out["fn_x0"] = np.array(0.25)
    out["fn_L0"] = np.asarray(L0_VECTOR)
    out["fn_tab_probe"] = np.stack([tabx[::500], taby[::500]])
    out["fn_ij0t83"] = starlord.Ij0t83(R_VECTOR * (np.pi / 0.25), tabx, taby)
    out["fn_dphi_highpass"] = starlord.dphi_highpass(R_VECTOR, 0.25, tabx, taby)
    out["fn_rodconan"] = np.stack([starlord.rodconan(R_VECTOR, L0) for L0 in L0_VECTOR])
    out["fn_dphi_lowpass"] = np.stack([starlord.dphi_lowpass(R_VECTOR, 0.25, L0, tabx, taby) for L0 in L0_VECTOR])
    x = R_VECTOR * (np.pi / 0.25)
    assert (x < np.exp(-3.0)).sum() >= 3 and (x > tabx[-1]).sum() >= 2 and ((x >= np.exp(-3.0)) & (x < tabx[-1])).sum() >= 10
    for L0 in L0_VECTOR:
        big = (2 * np.pi / L0) * R_VECTOR > 4.71239
        assert big.sum() >= 3 and (~big).sum() >= 3, L0
    # the coupling matrix of the production systems' kept actuators
    for tag, name in (("10x10", "production_sh_10x10_2m"), ("40x40", "production_sh_40x40_8m_3layers")):
        i1, j1, pitch, dim, coupling = kept_actuators(name)
        p_dm = types.SimpleNamespace(_ntotact=i1.size, coupling=coupling, _n1=1, _n2=dim, _i1=i1, _j1=j1, _pitch=pitch)
        Nact = create_nact_geom(p_dm)
        print("%s: %d kept actuators, pitch %g, support %d, %d non-zero couplings" % (tag, i1.size, pitch, dim, (Nact != 0).sum()))
        for k, v in (("i1", i1), ("j1", j1), ("pitch", pitch), ("dim", dim), ("coupling", coupling)):
            out["nact_%s_%s" % (tag, k)] = np.asarray(v)
        if i1.size <= 200:
            out["nact_%s_dense" % tag] = Nact
        else:
            m = sp.csr_matrix(Nact)
            out["nact_%s_data" % tag], out["nact_%s_indices" % tag], out["nact_%s_indptr" % tag] = m.data, m.indices, m.indptr
    path = os.path.join(ROOT, "tests", "golden", "groot.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
