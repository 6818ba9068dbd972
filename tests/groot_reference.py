"""An independent float64 restatement of the GROOT covariance model (guardians/groot.py, guardians/starlord.py) for the
tests of ao_marl_amd/groot.py.  It follows the reference's ORDER term by term -- four separation matrices and Caniso /
Cbp / Ccov per layer, the npts^2 double loop of the aliasing model, the twelve terms of dCmm, N^-1 C N^-1 then Tf . Tf^T
and pzt2tt . pzt2tt^T then P . P^T -- and deliberately NOT the telescoped, collapsed and pre-composed forms the product
uses.  `c` is a mapping with the keys VecRoket.save writes (tests/golden/groot.npz holds two, prefixed "A_" and "B_")."""
import numpy as np
import scipy.sparse as sp
from scipy.special import jv

RASC = 180. / np.pi * 3600.
COUNTS = {"ij0_series": 0, "ij0_table": 0, "rodconan_series": 0, "rodconan_asymptotic": 0}
_TAB = []


def case(z, name):
    """the datasets, attributes and reference outputs ("out_...") of case `name` of the golden file"""
    pre = name + "_"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def reset_counts():
    for k in COUNTS:
        COUNTS[k] = 0


def table():
    if not _TAB:
        n = 10000
        t = np.linspace(-4, 10, n)
        dt = (t[-1] - t[0]) / (n - 1)
        x0 = np.exp(-4.0)
        first = 0.75 * x0 ** (1. / 3) * (1 - x0 ** 2 / 112.)
        X = np.exp(t)
        f = np.exp(-t * (5. / 3.)) * (1 - jv(0, X))
        Y = np.zeros(n)
        Y[1:] = np.cumsum(0.5 * (f[:-1] + f[1:]))                 # the trapezoid rule
        _TAB.extend([X, Y * dt + first])
    return _TAB


def ij0t83(x):
    tabx, taby = table()
    x = np.asarray(x, dtype=np.float64)
    res = np.empty_like(x)
    small = x < np.exp(-3.0)
    COUNTS["ij0_series"] += int(small.sum())
    COUNTS["ij0_table"] += int((~small).sum())
    res[small] = 0.75 * x[small] ** (1. / 3) * (1 - x[small] ** 2 / 112.)
    res[~small] = np.interp(x[~small], tabx, taby)
    return res


def dphi_highpass(r, x0):
    r = np.asarray(r, dtype=np.float64)
    return r ** (5. / 3.) * (1.1183343328701949 - ij0t83(r * (np.pi / x0))) * (2 * (2 * np.pi) ** (8 / 3.) * 0.0228956)


GA = [0, 12.067619015983075, 5.17183672113560444, 0.795667187867016068, 0.0628158306210802181, 0.00301515986981185091,
      9.72632216068338833e-05, 2.25320204494595251e-06, 3.93000356676612095e-08, 5.34694362825451923e-10,
      5.83302941264329804e-12]
GMA = [-3.74878707653729304, -2.04479295083852408, -0.360845814853857083, -0.0313778969438136685, -0.001622994669507603,
       -5.56455315259749673e-05, -1.35720808599938951e-06, -2.47515152461894642e-08, -3.50257291219662472e-10,
       -3.95770950530691961e-12, -3.65327031259100284e-14]


def rodconan(r, L0):
    r = np.asarray(r, dtype=np.float64)
    res = np.zeros_like(r)
    x = (2 * np.pi / L0) * r
    big = x > 4.71239
    COUNTS["rodconan_asymptotic"] += int(big.sum())
    COUNTS["rodconan_series"] += int((~big).sum())
    xb = x[big]
    res[big] = 1.00563491799858928388289314170833 - 1.25331413731550012081 * np.exp(-xb) * xb ** (1. / 3.) * \
        (1.0 + (0.22222222222222222222 + (-0.08641975308641974829 + 0.08001828989483310284 / xb) / xb) / xb)
    xs = x[~big]
    x2a, q = xs ** (5. / 3.), xs * xs / 4.
    s, p = GMA[0] * x2a * 0.5, 0.5 * q
    for n in range(1, 11):
        s = s + (GMA[n] * x2a + GA[n]) * p
        p = p * q
    res[~big] = -s
    return res * (0.1716613621245709486 * L0 ** (5. / 3.))


def dphi_lowpass(r, x0, L0):
    return rodconan(r, L0) - dphi_highpass(r, x0)


def _s(c, k):
    return float(np.asarray(c[k], dtype=np.float64).reshape(-1)[0])


def _v(c, k):
    return np.atleast_1d(np.asarray(c[k], dtype=np.float64))


def actuators(c):
    p2m = _s(c, "_Param_tel__diam") / _s(c, "_Param_geom__pupdiam")
    pupshape = int(2 ** np.ceil(np.log2(_s(c, "_Param_geom__pupdiam")) + 1))
    return (_v(c, "dm.xpos") - pupshape / 2) * p2m, (_v(c, "dm.ypos") - pupshape / 2) * p2m


def subapertures(c):
    nsub = np.asarray(c["R"]).shape[1] // 2
    nssp = int(_s(c, "_Param_wfs__nxsub"))
    cobs = _s(c, "_Param_tel__cobs")
    x = np.linspace(-1, 1, nssp)
    x, y = np.meshgrid(x, x)
    r = np.sqrt(x * x + y * y)
    rorder = np.sort(r.reshape(nssp * nssp))
    ncentral = nssp * nssp - np.sum(r >= cobs, dtype=np.int32)
    validext = rorder[ncentral + nsub]
    ivalid = np.where((r < validext) & (r >= cobs))
    if "_Param_wfs___validsubsx" in c:                      # the sensor's own list, where the file has it
        npix = int(_s(c, "_Param_wfs__npix"))
        ivalid = (np.asarray(c["_Param_wfs___validsubsy"]) // npix, np.asarray(c["_Param_wfs___validsubsx"]) // npix)
    d = _s(c, "_Param_tel__diam") / nssp
    x = (np.arange(nssp) - nssp / 2) * d
    x, y = np.meshgrid(x, x)
    return x[ivalid], y[ivalid], d, nsub


def pzt2tt_f32(c):
    """the reference's float32 products (drax.get_IF hands out float32; groot.py:192-198)"""
    IF = sp.csr_matrix((np.asarray(c["IF.data"]), np.asarray(c["IF.indices"]), np.asarray(c["IF.indptr"]))).T
    T = np.asarray(c["TT"]).T.astype(np.float32).T              # get_IF's copy, transposed back: the same memory order
    N = IF.shape[0]
    deltaTT = T.T.dot(T) / N
    deltaF = IF.T.dot(T) / N
    return np.linalg.inv(deltaTT).dot(deltaF.T)


def pzt2tt_f64(c):
    IF = sp.csr_matrix((np.asarray(c["IF.data"], dtype=np.float64), np.asarray(c["IF.indices"]), np.asarray(c["IF.indptr"]))).T
    T = np.asarray(c["TT"], dtype=np.float64)
    return np.linalg.solve(T.T.dot(T), np.asarray(IF.T.dot(T)).T)


def ctt_actuators(c, speed=None, H=None, theta=None, r0=None, L0=None, gain=None):
    """the sum over the layers in actuator space, before any projection (:137-186): [na][na]"""
    lt, lw = _s(c, "tar_lambda"), _s(c, "_Param_wfs__Lambda")
    dt = _s(c, "_Param_loop__ittime")
    gain = _s(c, "_Param_controller__gain") if gain is None else float(gain)
    wx, wy = _s(c, "_Param_wfs__xpos"), _s(c, "_Param_wfs__ypos")
    r0 = (_s(c, "_Param_atmos__r0") if r0 is None else float(r0)) * (lt / lw) ** (6. / 5.)
    H = _v(c, "_Param_atmos__alt") if H is None else np.asarray(H, dtype=np.float64)
    L0 = _v(c, "_Param_atmos__L0") if L0 is None else np.asarray(L0, dtype=np.float64)
    speed = _v(c, "_Param_atmos__windspeed") if speed is None else np.asarray(speed, dtype=np.float64)
    theta = _v(c, "_Param_atmos__winddir") * np.pi / 180. if theta is None else np.asarray(theta, dtype=np.float64)
    frac = _v(c, "_Param_atmos__frac")
    xa, ya = actuators(c)
    n = xa.size
    xij = xa[None, :] - xa[:, None]
    yij = ya[None, :] - ya[:, None]
    fc = xa[1] - xa[0]
    Ccov, Caniso, Cbp = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    aht = np.arctan2(wy, wx)
    for l in range(int(_s(c, "_Param_atmos__nscreens"))):
        ht = np.hypot(wx, wy) / RASC * H[l]
        vdt = speed[l] * dt / gain
        M = np.hypot(xij, yij)
        Mv = np.hypot(xij - vdt * np.cos(theta[l]), yij - vdt * np.sin(theta[l]))
        Mh = np.hypot(xij - ht * np.cos(aht), yij - ht * np.sin(aht))
        Mhv = np.hypot(xij - vdt * np.cos(theta[l]) - ht * np.cos(aht), yij - vdt * np.sin(theta[l]) - ht * np.sin(aht))
        D = lambda m: dphi_lowpass(m, fc, L0[l])                                  # noqa: E731
        k = (1. / r0) ** (5. / 3.) * frac[l]
        Ccov += 0.5 * (D(Mhv) - D(Mh) - D(Mv) + D(M)) * k
        Caniso += 0.5 * (D(Mh) - D(M)) * k
        Cbp += 0.5 * (D(Mv) - D(M)) * k
    Sp = (lt / (2 * np.pi)) ** 2
    Ctt = (Caniso + Caniso.T) * Sp
    Ctt += (Cbp + Cbp.T) * Sp
    Ctt += (Ccov + Ccov.T) * Sp
    return Ctt


def cerr(c, modal=True, pzt2tt=None, **over):
    """compute_Cerr_cpu (:110-212); pzt2tt: the tip-tilt the stack array makes (default: the reference's float32 one)"""
    Ctt = ctt_actuators(c, **over)
    P, Btt = np.asarray(c["P"], dtype=np.float64), np.asarray(c["Btt"], dtype=np.float64)
    Tf = Btt[:-2, :-2].dot(P[:-2, :-2])
    p2t = pzt2tt_f32(c) if pzt2tt is None else pzt2tt
    N1 = np.linalg.inv(np.asarray(c["Nact"], dtype=np.float64))
    Ctt = N1.dot(Ctt).dot(N1)
    ttcomp = p2t.dot(Ctt).dot(p2t.T)
    Ctt = Tf.dot(Ctt).dot(Tf.T)
    out = np.zeros((Ctt.shape[0] + 2,) * 2)
    out[:-2, :-2] = Ctt
    out[-2:, -2:] = ttcomp
    return P.dot(out).dot(P.T) if modal else out


def simpson(n):
    if n % 2 == 0:
        raise ValueError("n must be odd")
    co = np.ones(n)
    if n > 1:
        co[1::2] = 4
        co[2:-1:2] = 2
    return co


def calias(c, slopes_space=False, modal=True, npts=3):
    """compute_Calias (:533-609): the npts^2 double loop"""
    x, y, d, nsub = subapertures(c)
    r0, lw = _s(c, "_Param_atmos__r0"), _s(c, "_Param_wfs__Lambda")
    scale = 0.5 * (1 / r0) ** (5 / 3)
    cc = (RASC * lw * 1e-6 / 2 / np.pi) / d ** 2
    xx = x[None, :] - x[:, None]
    yy = y[None, :] - y[:, None]
    co = simpson(npts)
    h = d / (npts - 1) if npts > 1 else 1
    Ca = np.zeros((2 * nsub, 2 * nsub))
    D = lambda a, b: dphi_highpass(np.hypot(a, b), d)                              # noqa: E731
    for k in range(npts):
        for p in range(npts):
            o = (k - p) * h
            Ca[:nsub, :nsub] += (D(xx - d, yy + o) + D(xx + d, yy + o) - 2 * D(xx, yy + o)) * co[k] * co[p]
            Ca[nsub:, nsub:] += (D(xx + o, yy - d) + D(xx + o, yy + d) - 2 * D(xx + o, yy)) * co[k] * co[p]
    if not slopes_space:
        R = np.asarray(c["R"], dtype=np.float64)
        Ca = R.dot(Ca).dot(R.T)
        if modal:
            P = np.asarray(c["P"], dtype=np.float64)
            Ca = P.dot(Ca).dot(P.T)
    return Ca * scale * cc ** 2 * (h / 3) ** 2


def dcmm(c, ws=None, wd=None, dk=1):
    """compute_dCmm (:792-903)"""
    x, y, d, nsub = subapertures(c)
    ws = _v(c, "_Param_atmos__windspeed") if ws is None else np.asarray(ws, dtype=np.float64)
    wd = _v(c, "_Param_atmos__winddir") if wd is None else np.asarray(wd, dtype=np.float64)
    dt = _s(c, "_Param_loop__ittime") * dk
    L0, frac = _v(c, "_Param_atmos__L0"), _v(c, "_Param_atmos__frac")
    r0, lw = _s(c, "_Param_atmos__r0"), _s(c, "_Param_wfs__Lambda")
    scale = 0.5 * (1 / r0) ** (5 / 3) * (RASC * lw * 1e-6 / 2 / np.pi) ** 2 / d ** 2
    xij = x[None, :] - x[:, None]
    yij = y[None, :] - y[:, None]
    out = np.zeros((2 * nsub, 2 * nsub))
    for k in range(ws.size):
        vx, vy = ws[k] * dt * np.cos(wd[k] / 180 * np.pi), ws[k] * dt * np.sin(wd[k] / 180 * np.pi)
        Rc = lambda a, b: rodconan(np.hypot(a, b), L0[k])                          # noqa: E731
        e = np.zeros_like(out)
        e[:nsub, :nsub] += Rc(-xij - d + vx, -yij + vy) + Rc(-xij + d + vx, -yij + vy) - 2 * Rc(-xij + vx, -yij + vy)
        e[:nsub, :nsub] -= Rc(xij - d + vx, yij + vy) + Rc(xij + d + vx, yij + vy) - 2 * Rc(xij + vx, yij + vy)
        e[nsub:, nsub:] += Rc(-xij + vx, -yij - d + vy) + Rc(-xij + vx, -yij + d + vy) - 2 * Rc(-xij + vx, -yij + vy)
        e[nsub:, nsub:] -= Rc(xij + vx, yij - d + vy) + Rc(xij + vx, yij + d + vy) - 2 * Rc(xij + vx, yij + vy)
        out += frac[k] * 0.25 * e
    return out * scale


def form_terms(px, py, taps):
    """(sum_t w F, sum_t |w F|) of a tap list in float64, [B][n][n] each: the yardstick of the form kernel's bound"""
    dx, dy = px[None, :] - px[:, None], py[None, :] - py[:, None]
    B, T = taps["w"].shape
    tot, mag = np.zeros((B,) + dx.shape), np.zeros((B,) + dx.shape)
    for b in range(B):
        for t in range(T):
            r = np.hypot(dx + taps["ox"][b, t], dy + taps["oy"][b, t])
            F = {0: lambda: dphi_lowpass(r, taps["x0"], taps["L0"][b, t]), 1: lambda: dphi_highpass(r, taps["x0"]),
                 2: lambda: rodconan(r, taps["L0"][b, t])}[taps["kind"]]()
            tot[b] += taps["w"][b, t] * F
            mag[b] += np.abs(taps["w"][b, t] * F)
    return tot, mag
