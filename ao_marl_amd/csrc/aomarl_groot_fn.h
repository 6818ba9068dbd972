// aomarl_groot_fn.h -- the scalar structure functions of the GROOT covariance model (reference: guardians/starlord.py
// :10-140), in double, for host and device alike: k_groot_form (aomarl_groot.hip) evaluates them per pair and tap, and
// groot_host_check.cpp runs the same text on the CPU.  The branch points are the reference's:
//   Ij0t83(x)      x < e^-3: the series 3/4 x^(1/3) (1 - x^2 / 112); otherwise linear interpolation in x on the table
//                  (GR_NTAB points, x = e^t, t from -4 to 10), clamped to the last entry beyond it (np.interp)
//   rodconan(r)    2 pi r / L0 > 4.71239: the asymptotic form; otherwise the 10-term series of the MacDonald function
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GR_HD __host__ __device__ __forceinline__
#else
#define GR_HD static inline
#endif

#define GR_NTAB 10000
#define GR_TMIN (-4.0)
#define GR_TMAX 10.0
#define GR_XSMALL 0.049787068367863944   // exp(-3.0)
#define GR_DPRF0 4.71239
#define GR_KIND_LOWPASS 0
#define GR_KIND_HIGHPASS 1
#define GR_KIND_RODCONAN 2

// tabx[j] = exp(t_j) and taby[j], GR_NTAB entries each (groot.tabulate_ij0)
GR_HD double gr_ij0t83(double x, const double *tabx, const double *taby) {
  if (x < GR_XSMALL) return 0.75 * pow(x, 1. / 3) * (1 - x * x / 112.);
  if (x >= tabx[GR_NTAB - 1]) return taby[GR_NTAB - 1];
  // the interval from the logarithm, then moved until tabx[j] <= x < tabx[j + 1] holds on the stored abscissae
  int j = (int)((log(x) - GR_TMIN) * ((GR_NTAB - 1) / (GR_TMAX - GR_TMIN)));
  j = j < 0 ? 0 : (j > GR_NTAB - 2 ? GR_NTAB - 2 : j);
  while (j > 0 && x < tabx[j]) j--;
  while (j < GR_NTAB - 2 && x >= tabx[j + 1]) j++;
  const double slope = (taby[j + 1] - taby[j]) / (tabx[j + 1] - tabx[j]);
  return slope * (x - tabx[j]) + taby[j];
}

GR_HD double gr_dphi_highpass(double r, double x0, const double *tabx, const double *taby) {
  return pow(r, 5. / 3.) * (1.1183343328701949 - gr_ij0t83(r * (M_PI / x0), tabx, taby)) *
         (2 * pow(2 * M_PI, 8 / 3.) * 0.0228956);
}

GR_HD double gr_asymp_macdo(double x) {
  const double k2 = 1.00563491799858928388289314170833, k3 = 1.25331413731550012081;
  const double a1 = 0.22222222222222222222, a2 = -0.08641975308641974829, a3 = 0.08001828989483310284;
  const double x_1 = 1. / x;
  return k2 - k3 * exp(-x) * pow(x, 1. / 3.) * (1.0 + x_1 * (a1 + x_1 * (a2 + x_1 * a3)));
}

GR_HD double gr_macdo(double x) {
  const double Ga[11] = {0, 12.067619015983075, 5.17183672113560444, 0.795667187867016068, 0.0628158306210802181,
                         0.00301515986981185091, 9.72632216068338833e-05, 2.25320204494595251e-06,
                         3.93000356676612095e-08, 5.34694362825451923e-10, 5.83302941264329804e-12};
  const double Gma[11] = {-3.74878707653729304, -2.04479295083852408, -0.360845814853857083, -0.0313778969438136685,
                          -0.001622994669507603, -5.56455315259749673e-05, -1.35720808599938951e-06,
                          -2.47515152461894642e-08, -3.50257291219662472e-10, -3.95770950530691961e-12,
                          -3.65327031259100284e-14};
  const double x2a = pow(x, 2. * (5. / 6.)), x22 = x * x / 4.;
  double x2n = 0.5;
  double s = Gma[0] * x2a;
  s *= x2n;
  x2n *= x22;
  for (int n = 1; n <= 10; n++) {
    s += (Gma[n] * x2a + Ga[n]) * x2n;
    x2n *= x22;
  }
  return s;
}

GR_HD double gr_rodconan(double r, double L0) {
  const double k1 = 0.1716613621245709486;
  const double dprf0 = (2 * M_PI / L0) * r;
  const double res = dprf0 > GR_DPRF0 ? gr_asymp_macdo(dprf0) : -gr_macdo(dprf0);
  return res * (k1 * pow(L0, 5. / 3.));
}

GR_HD double gr_dphi_lowpass(double r, double x0, double L0, const double *tabx, const double *taby) {
  return gr_rodconan(r, L0) - gr_dphi_highpass(r, x0, tabx, taby);
}

GR_HD double gr_eval(int kind, double r, double x0, double L0, const double *tabx, const double *taby) {
  if (kind == GR_KIND_HIGHPASS) return gr_dphi_highpass(r, x0, tabx, taby);
  if (kind == GR_KIND_RODCONAN) return gr_rodconan(r, L0);
  return gr_dphi_lowpass(r, x0, L0, tabx, taby);
}
