// The per-lane constants of the slopes-only frame kernel's four-product moments (aomarl_spot_dev.h:
// spot_qf_moments), built on the host in double precision.  Plain C++, no HIP, no library: the same table on
// every host (fixed sweep orders, fixed tie-breaks; the only library calls are sin, cos, sqrt).
//
// The two Toeplitz kernels of the moments (see the comment above SpotQf) factor through ONE 16-column basis:
//     M = 2 Phi^T Phi,   S = 2 Phi^T U Phi,
// Phi [32][16] with rows cos(theta_j x), sin(theta_j x), theta_j = 2 pi (j + 1/2) / 64, j = 0 .. 15, and U
// antisymmetric, coupling the two rows of a j with u_j = 1/2 + (j >> 1).  With the thin SVD Phi = R Sigma V^T:
//     H = sqrt(2) V Sigma          ->  M = H H^T
//     T = R^T U R (antisymmetric)  ->  S = H T H^T
// and with the canonical form T = Q Lambda Q^T (Q orthogonal, Lambda = 2 x 2 blocks [[0, t_k], [-t_k, 0]]) and
// H' = H Q:      M = H' H'^T,      S = H' Lambda H'^T.
// Nothing is divided by a small singular value (columns of H' that belong to small ones are just small).
#pragma once
#include <cmath>
#include <cstring>

namespace aomarl_qf4 {

constexpr int NX = 16;              // pupil pixels of a sub-aperture per axis = columns of the basis
constexpr int NF = 16;              // frequencies +-(j + 1/2) per axis
constexpr int NR = 2 * NF;          // rows of Phi

struct Basis {
  double H[NX][NX];                 // H'[x][a]: columns (2k, 2k + 1) are the pair of t[k]
  double t[NX / 2];                 // Lambda[2k][2k + 1] = t[k] = -Lambda[2k + 1][2k],  t[k] > 0
  double err_m, err_s;              // |H' H'^T - M| / |M|,  |H' Lambda H'^T - S| / |S|  (Frobenius)
};

// cyclic Jacobi on a symmetric n x n matrix: A <- diagonal, W <- eigenvectors in columns
inline void jacobi_sym(double (&A)[NX][NX], double (&W)[NX][NX]) {
  for (int i = 0; i < NX; i++)
    for (int j = 0; j < NX; j++) W[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 100; sweep++) {
    bool rotated = false;
    for (int p = 0; p < NX - 1; p++)
      for (int q = p + 1; q < NX; q++) {
        const double apq = A[p][q];
        if (std::fabs(apq) <= 1e-17 * std::sqrt(std::fabs(A[p][p] * A[q][q])) || apq == 0.0) continue;
        rotated = true;
        const double zeta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / std::sqrt(1.0 + tn * tn), sn = cs * tn;
        for (int k = 0; k < NX; k++) {            // columns p, q
          const double a = A[k][p], b = A[k][q];
          A[k][p] = cs * a - sn * b; A[k][q] = sn * a + cs * b;
        }
        for (int k = 0; k < NX; k++) {            // rows p, q
          const double a = A[p][k], b = A[q][k];
          A[p][k] = cs * a - sn * b; A[q][k] = sn * a + cs * b;
        }
        for (int k = 0; k < NX; k++) {
          const double a = W[k][p], b = W[k][q];
          W[k][p] = cs * a - sn * b; W[k][q] = sn * a + cs * b;
        }
      }
    if (!rotated) break;
  }
}

// false if the factorisation misses M or S by more than 1e-12 of their norm (checked against the closed forms)
inline bool build_basis(Basis &out) {
  const double PI = 3.14159265358979323846;
  double A[NR][NX], U[NR][NR];
  double V[NX][NX], u[NF];
  std::memset(U, 0, sizeof U);
  for (int j = 0; j < NF; j++) {
    const double th = 2.0 * PI * (j + 0.5) / 64.0;
    u[j] = 0.5 + (double)(j >> 1);
    for (int x = 0; x < NX; x++) { A[2 * j][x] = std::cos(th * x); A[2 * j + 1][x] = std::sin(th * x); }
    U[2 * j + 1][2 * j] = u[j]; U[2 * j][2 * j + 1] = -u[j];
  }
  // ---- one-sided Jacobi (Hestenes): A <- Phi V = R Sigma, columns orthogonal
  for (int i = 0; i < NX; i++)
    for (int j = 0; j < NX; j++) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 100; sweep++) {
    bool rotated = false;
    for (int p = 0; p < NX - 1; p++)
      for (int q = p + 1; q < NX; q++) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int k = 0; k < NR; k++) { al += A[k][p] * A[k][p]; be += A[k][q] * A[k][q]; ga += A[k][p] * A[k][q]; }
        if (std::fabs(ga) <= 1e-17 * std::sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / std::sqrt(1.0 + tn * tn), sn = cs * tn;
        for (int k = 0; k < NR; k++) {
          const double a = A[k][p], b = A[k][q];
          A[k][p] = cs * a - sn * b; A[k][q] = sn * a + cs * b;
        }
        for (int k = 0; k < NX; k++) {
          const double a = V[k][p], b = V[k][q];
          V[k][p] = cs * a - sn * b; V[k][q] = sn * a + cs * b;
        }
      }
    if (!rotated) break;
  }
  double H[NX][NX], sig[NX];
  for (int i = 0; i < NX; i++) {
    double n2 = 0.0;
    for (int k = 0; k < NR; k++) n2 += A[k][i] * A[k][i];
    sig[i] = std::sqrt(n2);
    if (!(sig[i] > 0.0)) return false;
    for (int k = 0; k < NR; k++) A[k][i] /= sig[i];              // A = R from here (unit columns)
    for (int x = 0; x < NX; x++) H[x][i] = std::sqrt(2.0) * V[x][i] * sig[i];
  }
  // ---- T = R^T U R, antisymmetric by construction; B = T^T T = -T^2 has the eigenvalues t_k^2, each twice
  double T[NX][NX], B[NX][NX], W[NX][NX];
  {
    double UR[NR][NX];
    for (int a = 0; a < NR; a++)
      for (int i = 0; i < NX; i++) {
        double s = 0.0;
        for (int b = 0; b < NR; b++) s += U[a][b] * A[b][i];
        UR[a][i] = s;
      }
    double G[NX][NX];
    for (int i = 0; i < NX; i++)
      for (int j = 0; j < NX; j++) {
        double s = 0.0;
        for (int a = 0; a < NR; a++) s += A[a][i] * UR[a][j];
        G[i][j] = s;
      }
    for (int i = 0; i < NX; i++)
      for (int j = 0; j < NX; j++) T[i][j] = 0.5 * (G[i][j] - G[j][i]);
  }
  for (int i = 0; i < NX; i++)
    for (int j = 0; j < NX; j++) {
      double s = 0.0;
      for (int k = 0; k < NX; k++) s += T[k][i] * T[k][j];
      B[i][j] = s;
    }
  for (int i = 0; i < NX; i++)
    for (int j = i + 1; j < NX; j++) B[i][j] = B[j][i] = 0.5 * (B[i][j] + B[j][i]);
  jacobi_sym(B, W);
  int idx[NX];
  for (int i = 0; i < NX; i++) idx[i] = i;
  for (int i = 1; i < NX; i++)                                  // insertion sort, descending, stable
    for (int j = i; j > 0 && B[idx[j]][idx[j]] > B[idx[j - 1]][idx[j - 1]]; j--) { const int s = idx[j]; idx[j] = idx[j - 1]; idx[j - 1] = s; }
  // every second eigenvector w spans its plane together with T w:  q_{2k+1} = w,  q_{2k} = T w / |T w|,  t_k = |T w|
  // (T q_{2k+1} = t_k q_{2k},  T q_{2k} = -t_k q_{2k+1}); each new vector is cleaned of the planes before it
  double Q[NX][NX];
  auto clean = [&](double (&v)[NX], int ncol) {
    for (int pass = 0; pass < 2; pass++)
      for (int a = 0; a < ncol; a++) {
        double d = 0.0;
        for (int i = 0; i < NX; i++) d += v[i] * Q[i][a];
        for (int i = 0; i < NX; i++) v[i] -= d * Q[i][a];
      }
    double n2 = 0.0;
    for (int i = 0; i < NX; i++) n2 += v[i] * v[i];
    return std::sqrt(n2);
  };
  for (int k = 0; k < NX / 2; k++) {
    double w[NX], v[NX];
    for (int i = 0; i < NX; i++) w[i] = W[i][idx[2 * k]];
    double n = clean(w, 2 * k);
    if (!(n > 0.5)) return false;
    int big = 0;                                                 // sign: the largest component positive
    for (int i = 1; i < NX; i++) if (std::fabs(w[i]) > std::fabs(w[big])) big = i;
    if (w[big] < 0.0) n = -n;
    for (int i = 0; i < NX; i++) { w[i] /= n; Q[i][2 * k + 1] = w[i]; }
    for (int i = 0; i < NX; i++) {
      double s = 0.0;
      for (int j = 0; j < NX; j++) s += T[i][j] * w[j];
      v[i] = s;
    }
    for (int i = 0; i < NX; i++) Q[i][2 * k] = 0.0;
    const double tk = clean(v, 2 * k + 2);                       // (also against w: T w is orthogonal to w)
    if (!(tk > 0.0)) return false;
    for (int i = 0; i < NX; i++) Q[i][2 * k] = v[i] / tk;
    out.t[k] = tk;
  }
  for (int x = 0; x < NX; x++)
    for (int a = 0; a < NX; a++) {
      double s = 0.0;
      for (int i = 0; i < NX; i++) s += H[x][i] * Q[i][a];
      out.H[x][a] = s;
    }
  // ---- against the closed forms  M[d] = 2 sum_j cos(theta_j d),  S[d] = 2 sum_j u_j sin(theta_j d),  d = x' - x
  double em = 0.0, es = 0.0, nm = 0.0, ns = 0.0;
  for (int xp = 0; xp < NX; xp++)
    for (int x = 0; x < NX; x++) {
      double m = 0.0, s = 0.0, hm = 0.0, hs = 0.0;
      for (int j = 0; j < NF; j++) {
        const double th = 2.0 * PI * (j + 0.5) / 64.0 * (double)(xp - x);
        m += 2.0 * std::cos(th); s += 2.0 * u[j] * std::sin(th);
      }
      for (int a = 0; a < NX; a++) hm += out.H[xp][a] * out.H[x][a];
      for (int k = 0; k < NX / 2; k++)
        hs += out.t[k] * (out.H[xp][2 * k] * out.H[x][2 * k + 1] - out.H[xp][2 * k + 1] * out.H[x][2 * k]);
      em += (hm - m) * (hm - m); nm += m * m;
      es += (hs - s) * (hs - s); ns += s * s;
    }
  out.err_m = std::sqrt(em / nm); out.err_s = std::sqrt(es / ns);
  return out.err_m <= 1e-12 && out.err_s <= 1e-12;
}

// Column of H' that lane column c (and accumulator row 4q + r, as i = 4q + r) carries: bits 0 and 1 swapped, so
// that the two columns of a pair sit in lanes c and c ^ 2 and the two rows of a pair in registers r and r + 2
// (the lower and the upper half of an accumulator: one packed product per half).
inline int lane_column(int c) { return (c & ~3) | ((c & 1) << 1) | ((c >> 1) & 1); }

// sys.qf_tab, [64 lanes][8] floats, lane = 16 q + c:
//   [0 .. 3]  h[s] = H'[4q + s][lane_column(c)]: the B operand of E H' and the A operand of H'^T (E H')
//   [4], [5]  -2 t_{2q}, -2 t_{2q+1}: rows (4q, 4q+1) = registers (0, 2) and rows (4q+2, 4q+3) = registers (1, 3)
//             of the lane's accumulator -> row 1 of the moments = -sum (Y - 7.5) I, whole
//   [6]       +-t_k of the lane's column, k = lane_column(c) >> 1, + for the even column of the pair
//             -> row 2 of the moments = sum (X - 7.5) I / 2
//   [7]       0
inline bool build_table(float (&tab)[64 * 8], Basis *basis = nullptr) {
  Basis b;
  const bool ok = build_basis(b);
  if (basis) *basis = b;
  if (!ok) return false;
  for (int lane = 0; lane < 64; lane++) {
    const int q = lane >> 4, a = lane_column(lane & 15);
    float *o = tab + 8 * lane;
    for (int s = 0; s < 4; s++) o[s] = (float)b.H[4 * q + s][a];
    o[4] = (float)(-2.0 * b.t[2 * q]); o[5] = (float)(-2.0 * b.t[2 * q + 1]);
    o[6] = (float)((a & 1) ? -b.t[a >> 1] : b.t[a >> 1]);
    o[7] = 0.f;
  }
  return true;
}

}  // namespace aomarl_qf4
