"""Checkers of the ROKET error breakdown (ao_marl_amd/roket.py, csrc/aomarl_roket.hip).

filter_bank_f64: the loop filters of the reference (guardians/roket_generalized_rl.py:189-284) and its covariance /
correlation table (cov_cor, :441-480) in NumPy, for ONE environment, on whole [n][nactu] histories as the reference
keeps them.  `dtype` is float64 for the checker proper; the same code in float32 is what the tests measure the
precision of the recursion with.

OracleRoket: the breakdown's call sequence (:286-376) over the CPU oracle (oracle/aoref.py) as it is.
"""
import numpy as np

NAMES = ("noise", "trunc", "alias", "H_com", "bp", "tomo", "zeta")


def filter_bank_f64(derr, E, F, ageom, B, G, rl_com, RD, P, Btt, g, gamma, nfiltered, delay, dtype=np.float64):
    """All inputs [n][nactu] (G, rl_com may be None: G = B, no policy).  Returns a dict of [n][nactu] histories:
    the seven contributors under NAMES plus noise_buf, trunc_buf, tomo_buf, mod_com, wf_com.

    Buffers are zero-filled and indexed with t - 1 and t - delay as the reference indexes them, so that for
    t < delay the negative index lands on rows not written yet: history before frame 0 is zero."""
    f = dtype
    derr, E, F, ageom, B = (np.asarray(a, dtype=f) for a in (derr, E, F, ageom, B))
    G = B if G is None else np.asarray(G, dtype=f)
    n, na = derr.shape
    assert n > delay >= 1
    rl = np.zeros((n, na), dtype=f) if rl_com is None else np.asarray(rl_com, dtype=f)
    RD, P, Btt = np.asarray(RD, dtype=f), np.asarray(P, dtype=f), np.asarray(Btt, dtype=f)
    g, gamma = f(g), f(gamma)
    gRD = g * gamma * RD                                                        # :161
    nm = P.shape[0]
    lo, hi = nm - nfiltered - 2, nm - 2                                         # modes[-nfiltered-2:-2]
    h = {k: np.zeros((n, na), dtype=f) for k in NAMES + ("noise_buf", "trunc_buf", "tomo_buf", "mod_com", "wf_com")}
    ageom_buf, rl_buf = np.zeros((n, na), dtype=f), np.zeros((n, na), dtype=f)   # histories too: row t written at frame t
    for t in range(n):
        d = t - delay
        h["noise_buf"][t] = derr[t] - E[t]                                      # :215
        h["noise"][t] = h["noise"][t - 1] - gRD.dot(h["noise"][d]) + g * h["noise_buf"][d]          # :217-218
        h["trunc_buf"][t] = E[t] - gamma * F[t]                                 # :228
        h["trunc"][t] = h["trunc"][t - 1] - gRD.dot(h["trunc"][d]) + g * h["trunc_buf"][d]          # :230-231
        ageom_buf[t] = ageom[t]                                                 # :243
        h["alias"][t] = h["alias"][t - 1] - gRD.dot(h["alias"][d]) + gamma * g * ageom_buf[d]       # :245-247
        modes = P.dot(B[t])                                                     # :258-264
        filt = np.zeros_like(modes)
        filt[lo:hi] = modes[lo:hi]
        modes[lo:hi] = 0
        h["H_com"][t] = Btt.dot(filt)
        h["mod_com"][t] = Btt.dot(modes)
        C = h["mod_com"][t] - h["mod_com"][t - 1]                               # :267-269
        h["bp"][t] = h["bp"][t - 1] - gRD.dot(h["bp"][d]) - C
        rl_buf[t] = rl[t]                                                       # :181
        h["zeta"][t] = h["zeta"][t - 1] - gRD.dot(h["zeta"][d]) + rl_buf[d]     # :190-192
        gm = P.dot(G[t])                                                        # :277-284
        gm[lo:hi] = 0
        h["wf_com"][t] = Btt.dot(gm)
        h["tomo_buf"][t] = h["mod_com"][t] - h["wf_com"][t]
        h["tomo"][t] = h["tomo"][t - 1] - gRD.dot(h["tomo"][d]) - g * gamma * RD.dot(h["tomo_buf"][d])
    return h


def cov_cor(hist, P, with_zeta=True, start=0):
    """cov_cor (:441-480) of histories {name: [n][nactu]} from frame `start` on: 7x7 with a policy, 6x6 without."""
    names = NAMES if with_zeta else NAMES[:6]
    P = np.asarray(P, dtype=np.float64)
    y = [P.dot(np.asarray(hist[k], dtype=np.float64)[start:].T) for k in names]       # [nmodes][n]
    n = len(names)
    cov, cor = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            cov[i, j] = cov[j, i] = np.sum(np.mean(y[i] * y[j], axis=1) - np.mean(y[i], axis=1) * np.mean(y[j], axis=1))
    s = np.diag(cov).reshape(n, 1)
    sst = s.dot(s.T)
    ok = np.where(sst)
    cor[ok] = cov[ok] / np.sqrt(sst[ok])
    return cov, cor


def moments(hist, P, start=0):
    """S1 [7][nmodes], S2 [28][nmodes] (pairs k <= l, k major) of y_k = P x_k in float64, and the frame count."""
    P = np.asarray(P, dtype=np.float64)
    y = [P.dot(np.asarray(hist[k], dtype=np.float64)[start:].T) for k in NAMES]
    S1 = np.stack([v.sum(axis=1) for v in y])
    S2 = np.stack([(y[k] * y[l]).sum(axis=1) for k in range(7) for l in range(k, 7)])
    return S1, S2, y[0].shape[1]


class OracleRoket(object):
    """error_breakdown (:286-376) over an OracleSim `o` and its OracleGeo `geo`, as they are.  breakdown() is called
    where the reference calls it: the frame imaged and controlled (o's next_part_one stages, geo.next_part_one_geo),
    the command not yet applied.  The oracle's slopes, frame counter and target phase are put back.  Inputs are
    recorded per frame; contributors() runs filter_bank_f64 on them."""

    def __init__(self, o, geo, IF, RD, P, Btt, nfiltered, gamma=1.0):
        from oracle import aoref
        from ao_marl_amd import modal
        self.o, self.geo, self.IF, self._modal = o, geo, IF, modal
        self.RD, self.P, self.Btt, self.nfiltered, self.gamma = RD, P, Btt, nfiltered, gamma
        s = o.s
        self.cmat = np.asarray(s.cmat, dtype=np.float64)
        self.lit = s.spupil.reshape(-1) > 0
        # mirrors of the geometric fit of the residual phase: own shapes, o's sensor phase
        scr = aoref.OracleSim.__new__(aoref.OracleSim)
        scr.__dict__.update(o.__dict__)
        scr.dm_shapes = [np.zeros((d.dim, d.dim), dtype=np.float32) for d in s.dms]
        self.scr = scr
        self.rec = {k: [] for k in ("derr", "E", "F", "ageom", "B", "fit")}

    def breakdown(self):
        o, s = self.o, self.o.s
        derr = -self.cmat.dot(o.slopes)
        if s.noise >= 0:                                           # :194-220
            slopes, frame, cube = o.slopes.copy(), o.frame, o.bincube.copy()
            o.raytrace_wfs(atm=True, dms=True, reset=True)
            o.comp_image(noise=False)
            o.do_centroids()
            E = -self.cmat.dot(o.slopes)
            o.slopes[:], o.frame = slopes, frame
            o.bincube[:] = cube
        else:
            E = derr.copy()
        o.raytrace_wfs(atm=True, dms=True, reset=True)             # :222-233
        F = -self.cmat.dot(o.slopes_geom())
        tar = o.tar_phase.copy()                                   # :235-247
        o.raytrace_target(atm=True, dms=True, reset=True)
        com = self._modal.geo_command(self.IF, o.tar_phase.reshape(-1)[self.lit]).astype(np.float32)
        o.tar_phase[:] = tar
        self.scr.wfs_phase = o.wfs_phase
        self.scr.comp_shapes(com)
        self.scr.raytrace_wfs(atm=False, dms=True, reset=False)
        ageom = -self.cmat.dot(o.slopes_geom())
        fit = self.geo.comp_strehl()[2]                            # :249-256
        for k, v in (("derr", derr), ("E", E), ("F", F), ("ageom", ageom), ("B", self.geo.com.astype(np.float64)),
                     ("fit", fit)):
            self.rec[k].append(np.array(v))
        return derr, E, F, ageom

    def contributors(self):
        r = {k: np.stack(v) for k, v in self.rec.items()}
        s = self.o.s
        return filter_bank_f64(r["derr"], r["E"], r["F"], r["ageom"], r["B"], None, None, self.RD, self.P, self.Btt,
                               float(s.gain), self.gamma, self.nfiltered, int(float(s.delay)) + 1)
