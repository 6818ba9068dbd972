"""A plain-loop restatement of the covariance of two-point slopes between directions, written from the definition and
independently of ao_marl_amd.tomography.slope_covariance: scalar loops over stars, axes, points, layers and signs, the
four phase samples of the two slopes written out, the structure function its own transcription of the von Karman form
(the MacDonald function K_{5/6} through scipy-free series and asymptote, the coefficients of the published expansion).

    s_e^a(i) = kappa [phi_l(u + h e) - phi_l(u - h e)] / d,  u = delta_al p_i + alt_l theta_a,  h = delta_al d / 2
    <(phi(x1) - phi(x2)) (phi(y1) - phi(y2))> = [D(x1 - y2) + D(x2 - y1) - D(x1 - y1) - D(x2 - y2)] / 2
"""
import math

ARCSEC = 2 * math.pi / (360 * 3600)
KAPPA = 1e-6 * 206265.0
_GA = (0, 12.067619015983075, 5.17183672113560444, 0.795667187867016068, 0.0628158306210802181, 0.00301515986981185091,
       9.72632216068338833e-05, 2.25320204494595251e-06, 3.93000356676612095e-08, 5.34694362825451923e-10,
       5.83302941264329804e-12)
_GMA = (-3.74878707653729304, -2.04479295083852408, -0.360845814853857083, -0.0313778969438136685, -0.001622994669507603,
        -5.56455315259749673e-05, -1.35720808599938951e-06, -2.47515152461894642e-08, -3.50257291219662472e-10,
        -3.95770950530691961e-12, -3.65327031259100284e-14)


def structure(r, L0):
    """the von Karman phase structure function for r0 = 1 m, rad^2 at 0.5 microns"""
    x = 2 * math.pi * r / L0
    if x > 4.71239:
        xi = 1.0 / x
        v = 1.00563491799858928388289314170833 - 1.25331413731550012081 * math.exp(-x) * x ** (1. / 3.) * (
            1.0 + xi * (0.22222222222222222222 + xi * (-0.08641975308641974829 + xi * 0.08001828989483310284)))
    else:
        xa, q = x ** (5. / 3.), x * x / 4.
        p = 0.5
        s = _GMA[0] * xa * p
        for n in range(1, 11):
            p *= q
            s += (_GMA[n] * xa + _GA[n]) * p
        v = -s
    return v * 0.1716613621245709486 * L0 ** (5. / 3.)


def covariance(px, py, d, stars_a, stars_b, layers, qx=None, qy=None):
    """(C, M): C[(2 a + e) n_a + i][(2 b + f) n_b + j] in arcsec^2 and M = sum |w D| of the same taps, lists of lists"""
    qx, qy = (px if qx is None else qx), (py if qy is None else qy)
    na, nb = len(px), len(qx)
    C = [[0.0] * (2 * nb * len(stars_b)) for _ in range(2 * na * len(stars_a))]
    M = [[0.0] * (2 * nb * len(stars_b)) for _ in range(2 * na * len(stars_a))]
    for a, (tax, tay, ha) in enumerate(stars_a):
        for b, (tbx, tby, hb) in enumerate(stars_b):
            for e in range(2):
                for f in range(2):
                    for i in range(na):
                        for j in range(nb):
                            c = m = 0.0
                            for alt, r0l, L0 in layers:
                                w = (KAPPA / d) ** 2 * r0l ** (-5. / 3.) * (0.5 / (2 * math.pi)) ** 2
                                da, db = 1.0 - alt / ha, 1.0 - alt / hb
                                u = [da * px[i] + alt * tax * ARCSEC, da * py[i] + alt * tay * ARCSEC]
                                v = [db * qx[j] + alt * tbx * ARCSEC, db * qy[j] + alt * tby * ARCSEC]
                                x1, x2, y1, y2 = list(u), list(u), list(v), list(v)
                                x1[e] += da * d / 2
                                x2[e] -= da * d / 2
                                y1[f] += db * d / 2
                                y2[f] -= db * d / 2
                                dist = lambda p, q: math.hypot(p[0] - q[0], p[1] - q[1])  # noqa: E731
                                terms = (-structure(dist(x1, y1), L0), structure(dist(x1, y2), L0),
                                         structure(dist(x2, y1), L0), -structure(dist(x2, y2), L0))
                                for t in terms:
                                    c += 0.5 * w * t
                                    m += abs(0.5 * w * t)
                            C[(2 * a + e) * na + i][(2 * b + f) * nb + j] = c
                            M[(2 * a + e) * na + i][(2 * b + f) * nb + j] = m
    return C, M
