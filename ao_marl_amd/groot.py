"""GROOT: the residual-error covariance MODELLED from the atmosphere's structure functions, without running a loop
(reference: guardians/groot.py; the structure functions: guardians/starlord.py).  The file it reads is what
roket.VecRoket.save writes.

tabulate_ij0, ij0t83, dphi_highpass, rodconan, dphi_lowpass   starlord.py:10-140, the same branch points
GrootModel          cerr (bandwidth + anisoplanatism, compute_Cerr_cpu :110-212), calias (compute_Calias :533-609), dcmm
                    (compute_dCmm :792-903) on csrc/aomarl_groot.hip when the device is a GPU; on the CPU the same
                    statement runs in float64 NumPy -- that statement is the feature's definition.  ca_gendron, cn,
                    otf_fitting (:300-454) are float64 NumPy on the host; psf composes them as compute_PSF does (:457-481).

The three covariances are one form over a point set p_i (actuators or sub-apertures) and a tap list:
    C[i][j] = sum_t w_t F_t(|p_j - p_i + o_t|)
  Cerr    per layer 1/2 w [D(r - s) + D(r + s) - 2 D(r)], D = dphi_lowpass(., pitch, L0), s = vdt u(theta) + Htheta u(angleht):
          the reference's Caniso + Cbp + Ccov telescope to D(r - s) - D(r), and (. + .^T) turns -s into +s
  Calias  the (k, p) double loop only sees k - p: 2 npts - 1 offsets, weights sum(coeff[|m|:] coeff[:npts - |m|])
  dCmm    six taps of rodconan per layer and block
The chain behind Cerr is linear in C, so its atmosphere-independent factors are composed once, in float64:
modal Cerr = (P[:, :-2] Tf N^-1) C (.)^T + (P[:, -2:] pzt2tt N^-1) C (.)^T, N = Nact."""
import ctypes as C

import numpy as np

from . import libaomarl as la
from . import psf_rec
from . import roket

RASC = 180. / np.pi * 3600.
NTAB, XSMALL, DPRF0 = 10000, np.exp(-3.0), 4.71239
LOWPASS, HIGHPASS, RODCONAN = 0, 1, 2
# evaluations per branch since the last reset (tests require all four to be taken)
branch_counts = {"ij0_series": 0, "ij0_table": 0, "rodconan_series": 0, "rodconan_asymptotic": 0}
_TABLE = None


# ------------------------------------------------------------------------------------------- structure functions
def tabulate_ij0():
    """(X, Y): the integral of t^(-8/3) (1 - J0(t)) from 0 to X on 10000 points X = e^t, t in [-4, 10] (:56-72)"""
    global _TABLE
    if _TABLE is None:
        from scipy.special import jv
        n = NTAB
        t = np.linspace(-4, 10, n)
        dt = (t[-1] - t[0]) / (n - 1)
        smallx = np.exp(-4.0)
        A = 0.75 * smallx ** (1. / 3) * (1 - smallx ** 2 / 112.)
        X = np.exp(t)
        Y = np.exp(-t * (5. / 3.)) * (1 - jv(0, X))
        Y[1:] = np.cumsum(Y[:-1] + np.diff(Y) / 2.)
        Y[0] = 0.
        _TABLE = (X, Y * dt + A)
    return _TABLE


def ij0t83(x, tabx=None, taby=None):
    """:36-53: the series below e^-3, linear interpolation in x on the table above, its last entry beyond the end"""
    if tabx is None:
        tabx, taby = tabulate_ij0()
    x = np.asarray(x, dtype=np.float64)
    small = x < XSMALL
    branch_counts["ij0_series"] += int(small.sum())
    branch_counts["ij0_table"] += int(x.size - small.sum())
    return np.where(small, 0.75 * x ** (1. / 3) * (1 - x ** 2 / 112.), np.interp(x, tabx, taby))


def dphi_highpass(r, x0, tabx=None, taby=None):
    """:10-21: the phase structure function above the cut-off 1 / (2 x0), to be scaled by r0^(-5/3)"""
    r = np.asarray(r, dtype=np.float64)
    return (r ** (5. / 3.)) * (1.1183343328701949 - ij0t83(r * (np.pi / x0), tabx, taby)) * \
        (2 * (2 * np.pi) ** (8 / 3.) * 0.0228956)


def _asymp_macdo(x):
    k2, k3 = 1.00563491799858928388289314170833, 1.25331413731550012081
    a1, a2, a3 = 0.22222222222222222222, -0.08641975308641974829, 0.08001828989483310284
    x_1 = 1. / x
    return k2 - k3 * np.exp(-x) * x ** (1. / 3.) * (1.0 + x_1 * (a1 + x_1 * (a2 + x_1 * a3)))


_GA = (0, 12.067619015983075, 5.17183672113560444, 0.795667187867016068, 0.0628158306210802181, 0.00301515986981185091,
       9.72632216068338833e-05, 2.25320204494595251e-06, 3.93000356676612095e-08, 5.34694362825451923e-10,
       5.83302941264329804e-12)
_GMA = (-3.74878707653729304, -2.04479295083852408, -0.360845814853857083, -0.0313778969438136685, -0.001622994669507603,
        -5.56455315259749673e-05, -1.35720808599938951e-06, -2.47515152461894642e-08, -3.50257291219662472e-10,
        -3.95770950530691961e-12, -3.65327031259100284e-14)


def _macdo(x):
    x2a = x ** (2. * (5. / 6.))
    x22 = x * x / 4.
    x2n = 0.5
    s = _GMA[0] * x2a
    s = s * x2n
    x2n = x2n * x22
    for n in range(1, 11):
        s = s + (_GMA[n] * x2a + _GA[n]) * x2n
        x2n = x2n * x22
    return s


def rodconan(r, L0):
    """:123-140: the von Karman structure function; 2 pi r / L0 > 4.71239: asymptotic form, otherwise the 10-term series"""
    r = np.asarray(r, dtype=np.float64)
    L0 = np.asarray(L0, dtype=np.float64)
    k1 = 0.1716613621245709486
    dprf0 = (2 * np.pi / L0) * r
    large = dprf0 > DPRF0
    branch_counts["rodconan_asymptotic"] += int(large.sum())
    branch_counts["rodconan_series"] += int(large.size - large.sum())
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        res = np.where(large, _asymp_macdo(np.where(large, dprf0, 1.0)), -_macdo(np.where(large, 0.0, dprf0)))
    return res * (k1 * L0 ** (5. / 3.))


def dphi_lowpass(r, x0, L0, tabx=None, taby=None):
    """:24-33"""
    return rodconan(r, L0) - dphi_highpass(r, x0, tabx, taby)


def simpson_coeff(n):
    """:612-630"""
    n = int(n)
    if n < 1 or n % 2 == 0:
        raise ValueError("groot: npts = %d: the Simpson rule (simpson_coeff) takes an odd number of points" % n)
    coeff = np.ones(n)
    if n > 1:
        coeff[1::2] = 4
        coeff[2:-1:2] = 2
    return coeff


def _evaluate(kind, r, x0, L0):
    if kind == HIGHPASS:
        return dphi_highpass(r, x0)
    if kind == RODCONAN:
        return rodconan(r, L0)
    return dphi_lowpass(r, x0, L0)


# ------------------------------------------------------------------------------------------- tap lists
def taps_cerr(w, sx, sy, x0, L0):
    """w, sx, sy, L0 [B][nl] -> dict(kind, x0, w, ox, oy, L0 [B][3 nl])"""
    z = np.zeros_like(w)
    st = lambda *a: np.stack(a, axis=2).reshape(w.shape[0], -1)          # noqa: E731
    return dict(kind=LOWPASS, x0=float(x0), w=st(0.5 * w, 0.5 * w, -w), ox=st(-sx, sx, z), oy=st(-sy, sy, z), L0=st(L0, L0, L0))


def taps_calias(w, d, npts, block):
    """w [B]: the overall factor; block "xx" / "yy" -> [B][3 (2 npts - 1)]"""
    coeff = simpson_coeff(npts)
    h = d / (npts - 1) if npts > 1 else 1.0
    ws, o1, o2 = [], [], []
    for m in range(-(npts - 1), npts):
        wm = (coeff[abs(m):] * coeff[:npts - abs(m)]).sum()
        ws += [wm, wm, -2.0 * wm]
        o1 += [-d, d, 0.0]                                                # along the slope's axis
        o2 += [m * h] * 3                                                 # across it
    ws, o1, o2 = (np.asarray(a)[None, :].repeat(w.shape[0], 0) for a in (ws, o1, o2))
    xx = block == "xx"
    return dict(kind=HIGHPASS, x0=float(d), w=ws * w[:, None], ox=o1 if xx else o2, oy=o2 if xx else o1, L0=np.ones_like(ws))


def taps_dcmm(w, vx, vy, d, L0, block):
    """w, vx, vy, L0 [B][nl] -> [B][6 nl]"""
    dx, dy = (d, 0.0) if block == "xx" else (0.0, d)
    st = lambda *a: np.stack(a, axis=2).reshape(w.shape[0], -1)          # noqa: E731
    q = 0.25 * w
    return dict(kind=RODCONAN, x0=float(d), w=st(q, q, -2 * q, -q, -q, 2 * q),
                ox=st(dx - vx, -dx - vx, -vx, -dx + vx, dx + vx, vx), oy=st(dy - vy, -dy - vy, -vy, -dy + vy, dy + vy, vy),
                L0=st(L0, L0, L0, L0, L0, L0))


def taps_of(spec):
    """spec: dict(model "cerr" | "calias_xx" | "calias_yy" | "dcmm_xx" | "dcmm_yy", x0, npts, w, sx, sy, L0 [B][nl]) -- what
    aomarl_groot_form takes -- -> the tap list the CPU statement sums"""
    m = spec["model"]
    if m == "cerr":
        return taps_cerr(spec["w"], spec["sx"], spec["sy"], spec["x0"], spec["L0"])
    if m.startswith("calias"):
        return taps_calias(spec["w"][:, 0], spec["x0"], spec["npts"], m[-2:])
    return taps_dcmm(spec["w"], spec["sx"], spec["sy"], spec["x0"], spec["L0"], m[-2:])


def form_cpu(px, py, taps, dtype=np.float64):
    """out [B][n][n] = sum_t w F(|p_j - p_i + o|), taps in order; the sum in float64, the result rounded to `dtype`"""
    dx, dy = px[None, :] - px[:, None], py[None, :] - py[:, None]
    B, T = taps["w"].shape
    out = np.zeros((B,) + dx.shape)
    for b in range(B):
        for t in range(T):
            r = np.sqrt((dx + taps["ox"][b, t]) ** 2 + (dy + taps["oy"][b, t]) ** 2)
            out[b] += taps["w"][b, t] * _evaluate(taps["kind"], r, taps["x0"], taps["L0"][b, t])
    return out.astype(dtype)


# ------------------------------------------------------------------------------------------- the model
KEYS = ("Nact", "dm.xpos", "dm.ypos", "P", "Btt", "R", "IF.data", "IF.indices", "IF.indptr", "TT", "tar_lambda",
        "_Param_atmos__r0", "_Param_atmos__alt", "_Param_atmos__L0", "_Param_atmos__windspeed", "_Param_atmos__winddir",
        "_Param_atmos__frac", "_Param_atmos__nscreens", "_Param_loop__ittime", "_Param_controller__gain",
        "_Param_wfs__xpos", "_Param_wfs__ypos", "_Param_wfs__Lambda", "_Param_wfs__nxsub", "_Param_tel__diam",
        "_Param_tel__cobs", "_Param_geom__pupdiam", "_Param_dm__nact")


def _pad4(a):
    """float32, rows padded to a multiple of 4 columns (the matrix kernel's 16-byte row pieces)"""
    a = np.asarray(a)
    out = np.zeros((a.shape[0], (a.shape[1] + 3) & ~3), dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


class GrootModel(object):
    """source: a VecRoket (kept histories), the .npz VecRoket.save wrote, or a mapping with its keys.  device None: the
    VecRoket's device, "cpu" for a file; "cpu" is the float64 statement (dtype=np.float32: the same statement with the
    device's rounding points -- the form rounded to float32, the projections in NumPy float32 -- what the GPU tests
    measure the arithmetic's own error with); a GPU device: csrc/aomarl_groot.hip."""

    def __init__(self, source, device=None, dtype=np.float64, batch_max=16):
        import scipy.sparse as sp
        self.d = d = psf_rec._as_dict(source)
        for k in KEYS:
            if k not in d:
                raise ValueError("groot: the source lacks %r (files written before the model existed do; a VecRoket "
                                 "writes it)" % k)
        if device is None:
            device = str(source.device) if isinstance(source, roket.VecRoket) else "cpu"
        self.device, self.dtype, self.batch_max = str(device), np.dtype(dtype), int(batch_max)
        a = lambda k: np.atleast_1d(np.asarray(d[k], dtype=np.float64))                # noqa: E731
        s = lambda k: float(a(k).reshape(-1)[0])                                       # noqa: E731
        self.nl = int(s("_Param_atmos__nscreens"))
        self.lam_tar, self.lam_wfs = s("tar_lambda"), s("_Param_wfs__Lambda")
        self.ittime, self.gain, self.r0 = s("_Param_loop__ittime"), s("_Param_controller__gain"), s("_Param_atmos__r0")
        self.wxpos, self.wypos = s("_Param_wfs__xpos"), s("_Param_wfs__ypos")
        self.diam, self.cobs, self.pupdiam = s("_Param_tel__diam"), s("_Param_tel__cobs"), s("_Param_geom__pupdiam")
        self.nssp, self.dm_nact = int(s("_Param_wfs__nxsub")), int(s("_Param_dm__nact"))
        self.alt, self.L0, self.speed = a("_Param_atmos__alt"), a("_Param_atmos__L0"), a("_Param_atmos__windspeed")
        self.winddir, self.frac = a("_Param_atmos__winddir"), a("_Param_atmos__frac")
        for k, v in (("alt", self.alt), ("L0", self.L0), ("windspeed", self.speed), ("winddir", self.winddir),
                     ("frac", self.frac)):
            if v.shape != (self.nl,):
                raise ValueError("groot: _Param_atmos__%s has %d entries, _Param_atmos__nscreens is %d" % (k, v.size, self.nl))
        # actuators, in metres from the pupil's centre (:131-136)
        p2m = self.diam / self.pupdiam
        pupshape = int(2 ** np.ceil(np.log2(self.pupdiam) + 1))
        self.xactu = (a("dm.xpos") - pupshape / 2) * p2m
        self.yactu = (a("dm.ypos") - pupshape / 2) * p2m
        self.pitch = float(self.xactu[1] - self.xactu[0])                              # :160
        self.na = na = self.xactu.size
        self.P, self.Btt, self.R = (np.asarray(d[k], dtype=np.float64) for k in ("P", "Btt", "R"))
        self.nm, self.nactu = self.P.shape
        Nact = np.asarray(d["Nact"], dtype=np.float64)
        if self.nactu != na + 2 or Nact.shape != (na, na) or self.Btt.shape != (self.nactu, self.nm):
            raise ValueError("groot: %d actuator positions, Nact %s, P %s, Btt %s do not agree" %
                             (na, Nact.shape, self.P.shape, self.Btt.shape))
        if not np.allclose(Nact, Nact.T, rtol=0, atol=1e-6 * np.abs(Nact).max()):
            raise ValueError("groot: Nact is not symmetric: the projection N^-1 C N^-1 (groot.py:202) is a congruence, "
                             "and the product's factors G C G^T, only for a symmetric coupling matrix")
        self.nsub = self.R.shape[1] // 2
        # the tip-tilt the stack array makes, in the reference's float32 (drax.get_IF hands out float32; :192-198)
        IF = sp.csr_matrix((np.asarray(d["IF.data"]), np.asarray(d["IF.indices"]), np.asarray(d["IF.indptr"])))
        T = np.asarray(d["TT"]).T.astype(np.float32)
        IF, T = IF.T, T.T
        N = IF.shape[0]
        deltaTT = T.T.dot(T) / N
        deltaF = IF.T.dot(T) / N
        self.pzt2tt = np.linalg.inv(deltaTT).dot(deltaF.T)
        N1 = np.linalg.inv(Nact)
        self.Tf = self.Btt[:-2, :-2].dot(self.P[:-2, :-2])
        pz, tt = self.Tf.dot(N1), self.pzt2tt.astype(np.float64).dot(N1)
        self.G = {"cerr_pzt": pz, "cerr_tt": tt, "cerr_modal_pzt": self.P[:, :-2].dot(pz),
                  "cerr_modal_tt": self.P[:, -2:].dot(tt), "R": self.R, "PR": self.P.dot(self.R)}
        # sub-apertures (:550-567)
        nssp = self.nssp
        x = np.linspace(-1, 1, nssp)
        x, y = np.meshgrid(x, x)
        r = np.sqrt(x * x + y * y)
        rorder = np.sort(r.reshape(nssp * nssp))
        ncentral = nssp * nssp - np.sum(r >= self.cobs, dtype=np.int32)
        validext = rorder[ncentral + self.nsub]
        self.ivalid = np.where((r < validext) & (r >= self.cobs))
        if "_Param_wfs___validsubsx" in d and "_Param_wfs___validsubsy" in d:
            # the sensor's own list, in the order of its slopes: the rule above is the reference's guess at it, and on the
            # 10 x 10 system it finds 60 of the 64 sub-apertures the illumination threshold keeps
            if "_Param_wfs__npix" not in d:
                raise ValueError("groot: the source lacks '_Param_wfs__npix'")
            npix = int(s("_Param_wfs__npix"))
            self.ivalid = (np.asarray(d["_Param_wfs___validsubsy"], dtype=np.int64) // npix,
                           np.asarray(d["_Param_wfs___validsubsx"], dtype=np.int64) // npix)
        self.dsub = self.diam / nssp
        x = (np.arange(nssp) - nssp / 2) * self.dsub
        x, y = np.meshgrid(x, x)
        self.xsub, self.ysub = x[self.ivalid], y[self.ivalid]
        if self.xsub.size != self.nsub:
            raise ValueError("groot: %d valid sub-apertures (the reference's rule on nxsub = %d, cobs = %g; a file with "
                             "_Param_wfs___validsubsx / ___validsubsy carries the sensor's own list), R has %d slopes" %
                             (self.xsub.size, nssp, self.cobs, self.R.shape[1]))
        self.ptr = None
        if self.device != "cpu":
            self._create()

    # ------------------------------------------------------------------------------------------ overrides
    def _layers(self, name, v, default, B):
        v = np.asarray(default if v is None else v, dtype=np.float64)
        if v.ndim == 0 or v.shape[-1] != self.nl or v.ndim > 2:
            raise ValueError("groot: %s has shape %s: %d layers (last axis), an optional batch axis in front" %
                             (name, v.shape, self.nl))
        if v.ndim == 2:
            B.append(v.shape[0])
        return v.reshape(-1, self.nl)

    def _scalar(self, name, v, default, B):
        v = np.asarray(default if v is None else v, dtype=np.float64)
        if v.ndim > 1:
            raise ValueError("groot: %s has shape %s: a number or one per batch entry" % (name, v.shape))
        if v.ndim == 1:
            B.append(v.shape[0])
        return v.reshape(-1, 1)

    @staticmethod
    def _batch(B):
        if len(set(B)) > 1:
            raise ValueError("groot: the overrides disagree on the batch size: %r" % (sorted(set(B)),))
        return (B[0], True) if B else (1, False)

    # ------------------------------------------------------------------------------------------ the three models
    def cerr_spec(self, speed=None, H=None, theta=None, r0=None, L0=None, gain=None):
        """(spec, batched) of compute_Cerr_cpu's sum over the layers (:145-186)"""
        B = []
        speed = self._layers("speed", speed, self.speed, B)
        H = self._layers("H", H, self.alt, B)
        theta = self._layers("theta", theta, self.winddir * np.pi / 180., B)
        L0 = self._layers("L0", L0, self.L0, B)
        r0 = self._scalar("r0", r0, self.r0, B)
        gain = self._scalar("gain", gain, self.gain, B)
        n, batched = self._batch(B)
        full = lambda v: np.broadcast_to(v, (n, v.shape[1])).astype(np.float64)        # noqa: E731
        speed, H, theta, L0, r0, gain = (full(v) for v in (speed, H, theta, L0, r0, gain))
        r0 = r0 * (self.lam_tar / self.lam_wfs) ** (6. / 5.)
        Htheta = np.linalg.norm([self.wxpos, self.wypos]) / RASC * H
        vdt = speed * self.ittime / gain
        angleht = np.arctan2(self.wypos, self.wxpos)
        sx = vdt * np.cos(theta) + Htheta * np.cos(angleht)
        sy = vdt * np.sin(theta) + Htheta * np.sin(angleht)
        w = (1. / r0) ** (5. / 3.) * self.frac[None, :] * (self.lam_tar / (2 * np.pi)) ** 2
        return dict(model="cerr", x0=self.pitch, npts=0, w=w, sx=sx, sy=sy, L0=L0), batched

    def cerr(self, modal=True, speed=None, H=None, theta=None, r0=None, L0=None, gain=None):
        """compute_Cerr_cpu (:110-212): [B][n][n] (B omitted when no override is batched), n = modes or actuators"""
        spec, batched = self.cerr_spec(speed, H, theta, r0, L0, gain)
        Cf = self.form("act", spec)
        if modal:
            out = self.sandwich("cerr_modal_pzt", Cf)
            out = self.sandwich("cerr_modal_tt", Cf, out, accumulate=True)
        else:                                   # the cross terms of the tip-tilt block stay zero (:205-207)
            out = self._zeros(Cf.shape[0], self.nactu)
            self.sandwich("cerr_pzt", Cf, out, at=0)
            self.sandwich("cerr_tt", Cf, out, at=self.na)
        out = self._host(out)
        return out if batched else out[0]

    def calias_specs(self, npts=3):
        """the XX and YY blocks' specs of compute_Calias (:558-563, :590-599, :609)"""
        simpson_coeff(npts)
        c = (RASC * self.lam_wfs * 1e-6 / 2 / np.pi) / self.dsub ** 2
        h = self.dsub / (npts - 1) if npts > 1 else 1.0
        w = np.array([[0.5 * (1 / self.r0) ** (5 / 3) * c ** 2 * (h / 3) ** 2]])
        return tuple(dict(model="calias_" + b, x0=self.dsub, npts=int(npts), w=w, sx=None, sy=None, L0=None)
                     for b in ("xx", "yy"))

    def calias_slopes(self, npts=3):
        """the slopes-space covariance, on the device when there is one: [1][2 nsub][2 nsub]"""
        return self.form2(*self.calias_specs(npts))

    def calias(self, slopes_space=False, modal=True, npts=3):
        """compute_Calias (:533-609)"""
        Ca = self.calias_slopes(npts)
        if not slopes_space:
            Ca = self.sandwich("PR" if modal else "R", Ca)
        return self._host(Ca)[0]

    def dcmm_specs(self, ws=None, wd=None, dk=1):
        """((XX spec, YY spec), batched) of compute_dCmm (:805-839, :859-860)"""
        B = []
        ws = self._layers("ws", ws, self.speed, B)
        wd = self._layers("wd", wd, self.winddir, B)
        n, batched = self._batch(B)
        ws, wd = (np.broadcast_to(v, (n, self.nl)).astype(np.float64) for v in (ws, wd))
        dt = self.ittime * dk
        scale = 0.5 * (1 / self.r0) ** (5 / 3) * (RASC * self.lam_wfs * 1e-6 / 2 / np.pi) ** 2 / self.dsub ** 2
        w = np.broadcast_to(self.frac[None, :] * scale, ws.shape).copy()
        vdt, ang = ws * dt, wd / 180 * np.pi
        vx, vy = vdt * np.cos(ang), vdt * np.sin(ang)
        L0 = np.broadcast_to(self.L0[None, :], ws.shape).copy()
        return tuple(dict(model="dcmm_" + b, x0=self.dsub, npts=0, w=w, sx=vx, sy=vy, L0=L0) for b in ("xx", "yy")), batched

    def dcmm(self, ws=None, wd=None, dk=1):
        """compute_dCmm (:792-903): d/dt(slopes) slopes^T, [B][2 nsub][2 nsub]; wd in degrees"""
        specs, batched = self.dcmm_specs(ws, wd, dk)
        out = self._host(self.form2(*specs))
        return out if batched else out[0]

    def form2(self, xx, yy):
        """the XX and YY blocks of a slopes-space covariance [B][2 nsub][2 nsub], zero elsewhere"""
        ns = self.nsub
        out = self._zeros(xx["w"].shape[0], 2 * ns)
        if self.ptr is None:
            out[:, :ns, :ns] = form_cpu(self.xsub, self.ysub, taps_of(xx), self.dtype)
            out[:, ns:, ns:] = form_cpu(self.xsub, self.ysub, taps_of(yy), self.dtype)
        else:
            self._form_native(xx, "sub", out, 0)
            self._form_native(yy, "sub", out, ns)
        return out

    def form(self, which, spec):
        """the form over the actuators ("act") or the sub-apertures ("sub"): [B][n][n] (device: [B][n][n padded to 4])"""
        px, py = (self.xactu, self.yactu) if which == "act" else (self.xsub, self.ysub)
        if self.ptr is None:
            return form_cpu(px, py, taps_of(spec), self.dtype)
        out = self._zeros(spec["w"].shape[0], px.size)
        self._form_native(spec, which, out, 0)
        return out

    def sandwich(self, name, Cf, out=None, at=0, accumulate=False):
        """out[:, at:at + m, at:at + m] (+)= G C G^T for the factor G = self.G[name]; out None: a new [B][m][m]"""
        G = self.G[name]
        m = G.shape[0]
        if self.ptr is not None:
            return self._sandwich_native(name, Cf, out, at, accumulate)
        f = self.dtype
        Gf = G.astype(f)
        r = np.stack([Gf.dot(c.astype(f)).dot(Gf.T) for c in Cf])
        if out is None:
            return r
        if accumulate:
            out[:, at:at + m, at:at + m] += r
        else:
            out[:, at:at + m, at:at + m] = r
        return out

    def _zeros(self, B, n):
        if self.ptr is None:
            return np.zeros((B, n, n), dtype=self.dtype)
        import torch
        return torch.zeros(B, n, (n + 3) & ~3, dtype=torch.float32, device=self.tdev)

    def _host(self, a):
        if isinstance(a, np.ndarray):
            return a
        return a[:, :, :a.shape[1]].cpu().numpy()

    # ------------------------------------------------------------------------------------------ host-only terms
    def ca_gendron(self, modal=True):
        """compute_Ca_cpu (:300-354): Gendron's aliasing model.  The stencil is laid over the same list of valid
        sub-apertures as calias and dcmm use (self.ivalid: the sensor's own where the file has it, else the reference's
        radial rule), so its rows and columns are R's slopes."""
        nsub, nssp = self.nsub, self.nssp
        xvalid, yvalid = self.ivalid[0] + 1, self.ivalid[1] + 1
        ivalid = (xvalid, yvalid)
        d = self.diam / (self.dm_nact - 1)
        r0 = self.r0 * (self.lam_tar / 0.5) ** (6. / 5.)
        scale = 0.23 * (d / r0) ** (5 / 3.) * (self.lam_tar * 1e-6 / (2 * np.pi * d)) ** 2 * RASC ** 2
        mask = np.zeros((nssp + 2, nssp + 2))
        Ca = np.identity(nsub * 2)
        for k in range(nsub):
            mask *= 0
            mask[xvalid[k], yvalid[k]] = 1
            mask[xvalid[k], yvalid[k] - 1] = -0.5
            mask[xvalid[k], yvalid[k] + 1] = -0.5
            Ca[k, :nsub] = mask[ivalid].flatten()
            mask *= 0
            mask[xvalid[k], yvalid[k]] = 1
            mask[xvalid[k] - 1, yvalid[k]] = -0.5
            mask[xvalid[k] + 1, yvalid[k]] = -0.5
            Ca[k + nsub, nsub:] = mask[ivalid].flatten()
        Ca = self.R.dot(Ca * scale).dot(self.R.T)
        return self.P.dot(Ca).dot(self.P.T) if modal else Ca

    def cn(self, model="data", modal=True, env=None):
        """compute_Cn_cpu (:357-413): "data": the covariance of the file's noise buffer (environment `env`, default the
        first kept one); "model": photon and read-out noise of the sensor's parameters"""
        d = self.d
        if model == "data":
            i = psf_rec._env_index(d, env) if env is not None else 0
            N = psf_rec._history(d, "noise", i)
            Cn = N.dot(N.T) / N.shape[1]
        elif model == "model":
            for k in ("_Param_wfs__npix", "_Param_wfs__noise", "_Param_wfs__zerop", "_Param_wfs__gsmag",
                      "_Param_wfs__optthroughput", "_Param_wfs__pixsize"):
                if k not in d:
                    raise ValueError("groot: the source lacks %r" % k)
            s = lambda k: float(np.asarray(d[k], dtype=np.float64).reshape(-1)[0])     # noqa: E731
            Cn = np.zeros(self.R.shape[1])
            noise = s("_Param_wfs__noise")
            if noise >= 0:
                Nph = s("_Param_wfs__zerop") * 10 ** (-0.4 * s("_Param_wfs__gsmag")) * s("_Param_wfs__optthroughput") * \
                    (self.diam / self.nssp) ** 2. * self.ittime
                r0 = (self.lam_wfs / 0.5) ** (6.0 / 5.0) * self.r0
                sig = (np.pi ** 2 / 2) * (1 / Nph) * (1. / r0) ** 2
                sig = sig * ((self.lam_wfs * 1e-6) / (2 * np.pi)) ** 2 * RASC ** 2
                Ns = s("_Param_wfs__npix")
                Nd = (self.lam_wfs * 1e-6) * RASC / s("_Param_wfs__pixsize")
                sigphi = (np.pi ** 2 / 3.0) * (1 / Nph ** 2) * noise ** 2 * Ns ** 2 * (Ns / Nd) ** 2
                sigsh = sigphi * ((self.lam_wfs * 1e-6) / (2 * np.pi)) ** 2 * RASC ** 2
                Cn[:] = sig + sigsh
            Cn = self.R.dot(np.diag(Cn)).dot(self.R.T)
        else:
            raise ValueError("groot: model = %r: \"data\" or \"model\"" % (model,))
        return self.P.dot(Cn).dot(self.P.T) if modal else Cn

    def otf_fitting(self, otftel):
        """compute_OTF_fitting (:416-454): (otf_fit, psf_fit) from dphi_highpass at the actuator pitch"""
        if "spup" not in self.d:
            raise ValueError("groot: the source lacks 'spup'")
        spup = np.asarray(self.d["spup"])
        otftel = np.asarray(otftel, dtype=np.float64)
        r0 = self.r0 * (self.lam_tar / 0.5) ** (6. / 5.)
        N = psf_rec.fft_size(spup.shape[0])
        if otftel.shape != (N, N):
            raise ValueError("groot: otftel is %s, the pupil's transform size is %d" % (otftel.shape, N))
        mask = np.ones((N, N))
        mask[np.where(otftel < 1e-5)] = 0
        x = (np.arange(N) - N / 2) * (self.diam / self.pupdiam)
        r = np.sqrt(x[:, None] * x[:, None] + x[None, :] * x[None, :])
        dphi = np.fft.fftshift(dphi_highpass(r, self.diam / (self.dm_nact - 1)) * (1 / r0) ** (5 / 3.))
        otf_fit = np.exp(-0.5 * dphi) * mask
        otf_fit = otf_fit / otf_fit.max()
        psf_fit = np.fft.fftshift(np.real(np.fft.ifft2(otftel * otf_fit)))
        psf_fit *= (N * N / float(np.where(spup)[0].shape[0]))
        return otf_fit, psf_fit

    @property
    def stroke_scale(self):
        """1 / unitpervolt^2 of the stack array, or None when the file does not say (_Param_dm__unitpervolt).  Nact^-1
        (:200-202) turns phase at the actuators into commands of influence functions with UNIT peak; a mirror whose
        influence functions peak at `unitpervolt` takes commands 1 / unitpervolt times larger, which the reference's Cerr
        does not know: on the production parameter sets (unitpervolt = 0.01) it comes out 1e4 below the volts^2 that P,
        Cn and Calias are in."""
        if "_Param_dm__unitpervolt" not in self.d:
            return None
        return 1.0 / float(np.asarray(self.d["_Param_dm__unitpervolt"], dtype=np.float64).reshape(-1)[0]) ** 2

    def cee(self, env=None, noise="data", cerr_scale=1.0):
        """Cerr . cerr_scale + Cn + Calias in the modal basis (:469-472).  cerr_scale = 1 is the reference's sum as it
        stands; see stroke_scale for what it leaves out when the mirror's unitpervolt is not 1."""
        return self.cerr() * float(cerr_scale) + self.cn(noise, env=env) + self.calias()

    def psf(self, env=None, noise="data", rec=None, cerr_scale=1.0):
        """compute_PSF (:457-481): the model's covariance through the Vii reconstruction, times the fitting OTF:
        dict(psf, strehl, otf2, otf_fit, otftel, cee).  With cerr_scale = 1 (the reference's sum) and unitpervolt = 0.01
        the bandwidth / anisoplanatism term is 1e4 below the other two and the PSF is in effect that of noise, aliasing
        and fitting alone; cerr_scale = self.stroke_scale puts Cerr into the commands' unit."""
        if rec is None:
            _, rec = psf_rec.from_source(self.d, device=self.device, dtype=self.dtype if self.device == "cpu" else np.float64)
        cee = self.cee(env, noise, cerr_scale)
        otf_fit, _ = self.otf_fitting(rec.tel["otftel"])
        r = rec.reconstruct(cee, otf_fit * rec.tel["otftel"])
        return dict(psf=r["psf"], strehl=r["strehl"], otf2=r["otf2"], otf_fit=otf_fit, otftel=r["otftel"], cee=cee)

    # ------------------------------------------------------------------------------------------ the native path
    def _create(self):
        import torch
        if not torch.cuda.is_available():
            raise la.AomarlError("GrootModel(device=%r) needs a GPU; device=\"cpu\" is the float64 statement" % self.device)
        self.lib = la.load()
        self.tdev = torch.device(self.device)
        tabx, taby = (np.ascontiguousarray(t, dtype=np.float64) for t in tabulate_ij0())
        d = la.GrootDesc()
        d.n_max, d.batch_max = max(self.na, self.nsub), self.batch_max
        d.m_max, d.k_max = self.nactu, max(self.na, 2 * self.nsub)
        d.tabx, d.taby = la.dptr(tabx), la.dptr(taby)
        ptr = C.c_void_p()
        with torch.cuda.device(self.tdev):
            la.check(self.lib.aomarl_groot_create(C.byref(d), C.byref(ptr)))
        self.ptr = ptr
        f64 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=self.tdev)    # noqa: E731
        self.pts = {"act": (f64(self.xactu), f64(self.yactu)), "sub": (f64(self.xsub), f64(self.ysub))}
        self.Gd = {k: torch.as_tensor(_pad4(v), device=self.tdev) for k, v in self.G.items()}

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.aomarl_groot_destroy(self.ptr)
            self.ptr = None

    MODELS = {"cerr": la.GROOT_CERR, "calias_xx": la.GROOT_CALIAS_XX, "calias_yy": la.GROOT_CALIAS_YY,
              "dcmm_xx": la.GROOT_DCMM_XX, "dcmm_yy": la.GROOT_DCMM_YY}

    def _form_native(self, spec, which, out, at):
        """out[b][at + i][at + j] of a device tensor [B][n][ld] (aomarl_groot_form)"""
        px, py = self.pts[which]
        B = spec["w"].shape[0]
        if B > self.batch_max:
            raise ValueError("groot: a batch of %d, the model was built with batch_max = %d" % (B, self.batch_max))
        f = la.GrootFormDesc()
        f.model, f.batch, f.nlayers, f.npts, f.x0 = self.MODELS[spec["model"]], B, spec["w"].shape[1], spec["npts"], spec["x0"]
        keep = {k: np.ascontiguousarray(spec[k], dtype=np.float64) for k in ("w", "sx", "sy", "L0") if spec[k] is not None}
        for k, v in keep.items():
            setattr(f, k, la.dptr(v))
        n, ld = px.numel(), out.shape[2]
        base = out.data_ptr() + 4 * (at * ld + at)
        sm = la.raw_stream(self.tdev)
        la.check(self.lib.aomarl_groot_form(self.ptr, C.byref(f), px.data_ptr(), py.data_ptr(), n, base, ld,
                                            out.shape[1] * ld, sm))

    def _sandwich_native(self, name, Cf, out, at, accumulate):
        import torch
        G = self.Gd[name]
        m, n = self.G[name].shape
        B = Cf.shape[0]
        if out is None:
            out = torch.empty(B, m, (m + 3) & ~3, dtype=torch.float32, device=self.tdev)
        sm = la.raw_stream(self.tdev)
        ld = out.shape[2]
        for b in range(B):
            la.check(self.lib.aomarl_groot_sandwich(self.ptr, G.data_ptr(), G.shape[1], m, Cf[b].data_ptr(), Cf.shape[2], n,
                                                    out[b].data_ptr() + 4 * (at * ld + at), ld, 1 if accumulate else 0, sm))
        return out
