// modal_host.h -- the dense part of the modal solve: Rayleigh-Ritz on Gram matrices of at most 96 x 96, on
// the host in plain C++ (Cholesky + cyclic Jacobi; the library links no LAPACK).  Mirrors tests/modal_np.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace tlfea {
namespace modal {

constexpr double kCholPivotMin = 1e-10;  // smallest pivot of the unit-diagonal Gram matrix the Cholesky path accepts
constexpr double kSvqbDrop = 1e-12;      // SVQB: directions below this share of the largest eigenvalue are dropped

// lower Cholesky factor of the k x k matrix G (row-major) into L; false when a pivot falls to pivot_min or below
inline bool cholesky_lower(int k, const std::vector<double>& G, double pivot_min, std::vector<double>& L) {
  L.assign((size_t)k * k, 0.0);
  for (int j = 0; j < k; j++) {
    double d = G[(size_t)j * k + j];
    for (int t = 0; t < j; t++) d -= L[(size_t)j * k + t] * L[(size_t)j * k + t];
    if (!(d > pivot_min)) return false;
    const double ljj = std::sqrt(d);
    L[(size_t)j * k + j] = ljj;
    for (int i = j + 1; i < k; i++) {
      double v = G[(size_t)i * k + j];
      for (int t = 0; t < j; t++) v -= L[(size_t)i * k + t] * L[(size_t)j * k + t];
      L[(size_t)i * k + j] = v / ljj;
    }
  }
  return true;
}

// eigenvalues (ascending) and eigenvectors (columns of V, row-major k x k) of the symmetric matrix A: cyclic Jacobi
inline void jacobi_eigh(int k, std::vector<double> A, std::vector<double>& w, std::vector<double>& V) {
  V.assign((size_t)k * k, 0.0);
  for (int i = 0; i < k; i++) V[(size_t)i * k + i] = 1.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < k; i++) {
      diag += A[(size_t)i * k + i] * A[(size_t)i * k + i];
      for (int j = 0; j < i; j++) off += A[(size_t)i * k + j] * A[(size_t)i * k + j];
    }
    if (off == 0.0 || std::sqrt(off) <= 1e-17 * std::sqrt(diag)) break;
    for (int p = 0; p < k - 1; p++)
      for (int q = p + 1; q < k; q++) {
        const double apq = A[(size_t)p * k + q];
        if (apq == 0.0) continue;
        const double app = A[(size_t)p * k + p], aqq = A[(size_t)q * k + q];
        if (std::fabs(apq) <= 1e-300) continue;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = std::isinf(theta) ? 0.0
                                           : (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int i = 0; i < k; i++) {  // columns p, q
          const double aip = A[(size_t)i * k + p], aiq = A[(size_t)i * k + q];
          A[(size_t)i * k + p] = c * aip - s * aiq;
          A[(size_t)i * k + q] = s * aip + c * aiq;
        }
        for (int i = 0; i < k; i++) {  // rows p, q
          const double api = A[(size_t)p * k + i], aqi = A[(size_t)q * k + i];
          A[(size_t)p * k + i] = c * api - s * aqi;
          A[(size_t)q * k + i] = s * api + c * aqi;
        }
        for (int i = 0; i < k; i++) {
          const double vip = V[(size_t)i * k + p], viq = V[(size_t)i * k + q];
          V[(size_t)i * k + p] = c * vip - s * viq;
          V[(size_t)i * k + q] = s * vip + c * viq;
        }
      }
  }
  std::vector<int> order(k);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[(size_t)a * k + a] < A[(size_t)b * k + b]; });
  w.resize(k);
  std::vector<double> Vs((size_t)k * k);
  for (int c = 0; c < k; c++) {
    w[c] = A[(size_t)order[c] * k + order[c]];
    for (int i = 0; i < k; i++) Vs[(size_t)i * k + c] = V[(size_t)i * k + order[c]];
  }
  V.swap(Vs);
}

// The n_want pairs of GM c = theta GA c with the largest theta (k x k, row-major, symmetrised here; GA positive definite
// up to rank loss of the basis): theta descending, C [k][n_got] with C^T GA C = I.  Returns n_got (<= n_want), 0 when GA
// has a non-positive diagonal entry.
inline int rayleigh_ritz(int k, std::vector<double> GA, std::vector<double> GM, int n_want, std::vector<double>& theta,
                         std::vector<double>& C) {
  for (int i = 0; i < k; i++)
    for (int j = 0; j < i; j++) {
      GA[(size_t)i * k + j] = GA[(size_t)j * k + i] = 0.5 * (GA[(size_t)i * k + j] + GA[(size_t)j * k + i]);
      GM[(size_t)i * k + j] = GM[(size_t)j * k + i] = 0.5 * (GM[(size_t)i * k + j] + GM[(size_t)j * k + i]);
    }
  std::vector<double> d(k);
  for (int i = 0; i < k; i++) {
    if (!(GA[(size_t)i * k + i] > 0.0)) return 0;
    d[i] = 1.0 / std::sqrt(GA[(size_t)i * k + i]);
  }
  std::vector<double> B((size_t)k * k), L, Q;
  for (int i = 0; i < k; i++)
    for (int j = 0; j < k; j++) B[(size_t)i * k + j] = GA[(size_t)i * k + j] * d[i] * d[j];
  int r = 0;  // columns of Q (k x r), Q^T GA Q = I
  if (cholesky_lower(k, B, kCholPivotMin, L)) {
    // Q = D L^-T: column c of L^-T by back substitution of L^T x = e_c
    r = k;
    Q.assign((size_t)k * k, 0.0);
    for (int c = 0; c < k; c++) {
      for (int i = c; i >= 0; i--) {
        double v = (i == c) ? 1.0 : 0.0;
        for (int t = i + 1; t <= c; t++) v -= L[(size_t)t * k + i] * Q[(size_t)t * k + c];
        Q[(size_t)i * k + c] = v / L[(size_t)i * k + i];
      }
    }
    for (int i = 0; i < k; i++)
      for (int c = 0; c < k; c++) Q[(size_t)i * k + c] *= d[i];
  } else {
    std::vector<double> w, V;
    jacobi_eigh(k, B, w, V);
    std::vector<int> keep;
    for (int c = 0; c < k; c++)
      if (w[c] > kSvqbDrop * w[k - 1]) keep.push_back(c);
    r = (int)keep.size();
    Q.assign((size_t)k * r, 0.0);
    for (int i = 0; i < k; i++)
      for (int c = 0; c < r; c++) Q[(size_t)i * r + c] = V[(size_t)i * k + keep[c]] / std::sqrt(w[keep[c]]) * d[i];
  }
  if (r == 0) return 0;
  // T = Q^T GM Q
  std::vector<double> GQ((size_t)k * r, 0.0), T((size_t)r * r, 0.0);
  for (int i = 0; i < k; i++)
    for (int t = 0; t < k; t++) {
      const double g = GM[(size_t)i * k + t];
      if (g == 0.0) continue;
      for (int c = 0; c < r; c++) GQ[(size_t)i * r + c] += g * Q[(size_t)t * r + c];
    }
  for (int a = 0; a < r; a++)
    for (int i = 0; i < k; i++) {
      const double qa = Q[(size_t)i * r + a];
      if (qa == 0.0) continue;
      for (int c = 0; c < r; c++) T[(size_t)a * r + c] += qa * GQ[(size_t)i * r + c];
    }
  for (int a = 0; a < r; a++)
    for (int c = 0; c < a; c++) T[(size_t)a * r + c] = T[(size_t)c * r + a] = 0.5 * (T[(size_t)a * r + c] + T[(size_t)c * r + a]);
  std::vector<double> w, Z;
  jacobi_eigh(r, T, w, Z);
  const int got = std::min(n_want, r);
  theta.resize(got);
  C.assign((size_t)k * got, 0.0);
  for (int c = 0; c < got; c++) {
    const int src = r - 1 - c;  // largest first
    theta[c] = w[src];
    for (int i = 0; i < k; i++) {
      double v = 0.0;
      for (int t = 0; t < r; t++) v += Q[(size_t)i * r + t] * Z[(size_t)t * r + src];
      C[(size_t)i * got + c] = v;
    }
  }
  return got;
}

}  // namespace modal
}  // namespace tlfea
