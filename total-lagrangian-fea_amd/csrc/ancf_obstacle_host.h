// ancf_obstacle_host.h -- host side of the rigid obstacles on the ANCF kinds (DESIGN 3e'): the 32 sample points of an
// element, their shape values (one table per distinct (L, W, H)) and their weights.  Included by
// obstacle_api.hip and, through ancf_load_host.h, loads_api.hip.
#pragma once
#include <array>
#include <cmath>
#include <map>
#include <vector>

#include "ancf_host.h"

namespace tlfea {
namespace ancf {

struct SamplePoint {
  double xi, eta, zeta, qw;  // normalised coordinates, quadrature weight
  int d0, d1;                // the two derivative directions that span the face (0 xi, 1 eta, 2 zeta)
};

// Shell (S = 16): faces zeta = -1, +1, each the 4 x 4 Gauss-Legendre rule in (xi, eta): p = face * 16 + ixi * 4 + ieta.
// Beam (S = 8): faces eta = -1, +1, zeta = -1, +1, each 4 Gauss points along xi and 2 across: p = face * 8 + ixi * 2 + k.
// The thin edge faces of a shell and the end caps of a beam carry no points.
inline std::array<SamplePoint, 32> sample_points(int S) {
  const double g4[4] = {-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526};
  const double w4[4] = {0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538};
  const double g2[2] = {-0.5773502691896257, 0.5773502691896257};
  std::array<SamplePoint, 32> pts;
  if (S == 16) {
    for (int f = 0; f < 2; f++)
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) pts[f * 16 + i * 4 + j] = {g4[i], g4[j], f ? 1.0 : -1.0, w4[i] * w4[j], 0, 1};
  } else {
    for (int f = 0; f < 4; f++)
      for (int i = 0; i < 4; i++)
        for (int k = 0; k < 2; k++) {
          const double sgn = (f & 1) ? 1.0 : -1.0;
          pts[f * 8 + i * 2 + k] = f < 2 ? SamplePoint{g4[i], sgn, g2[k], w4[i], 0, 2}
                                         : SamplePoint{g4[i], g2[k], sgn, w4[i], 0, 1};
        }
  }
  return pts;
}

struct ObstacleSetup {
  std::vector<int> cls;      // [E]
  std::vector<double> sval;  // [n_class][32][S]
  std::vector<double> w;     // [E][32]
};

// conn_cm [S][E]; Binv [E][S*S] column-major; xj/yj/zj the reference coefficients
inline ObstacleSetup obstacle_setup(int S, int E, const std::vector<int>& conn_cm, const std::vector<double>& Lv,
                                    const std::vector<double>& Wv, const std::vector<double>& Hv,
                                    const std::vector<double>& Binv, const double* xj, const double* yj,
                                    const double* zj) {
  const auto pts = sample_points(S);
  const Basis B = basis(S);
  ObstacleSetup out;
  out.cls.resize(E);
  out.w.resize((size_t)E * 32);
  std::map<std::array<double, 3>, int> seen;
  for (int e = 0; e < E; e++) {
    const std::array<double, 3> key = {Lv[e], Wv[e], Hv[e]};
    auto it = seen.find(key);
    const double* Bi = &Binv[(size_t)e * S * S];
    if (it == seen.end()) {
      it = seen.emplace(key, (int)seen.size()).first;
      out.sval.resize(seen.size() * 32 * S);
      double* tab = &out.sval[(size_t)it->second * 32 * S];
      for (int p = 0; p < 32; p++) {
        double b[16];
        eval(B, Lv[e] * pts[p].xi / 2, Wv[e] * pts[p].eta / 2, Hv[e] * pts[p].zeta / 2, 0, b);
        for (int i = 0; i < S; i++) {
          double a = 0.0;
          for (int j = 0; j < S; j++) a += Bi[(size_t)j * S + i] * b[j];
          tab[(size_t)p * S + i] = a;
        }
      }
    }
    out.cls[e] = it->second;
    for (int p = 0; p < 32; p++) {
      double ds[3][16], t[2][3] = {{0, 0, 0}, {0, 0, 0}};
      ds_dxi(S, Bi, Lv[e], Wv[e], Hv[e], pts[p].xi, pts[p].eta, pts[p].zeta, ds);
      for (int a = 0; a < S; a++) {
        const int id = conn_cm[(size_t)a * E + e];
        const double X[3] = {xj[id], yj[id], zj[id]};
        for (int c = 0; c < 3; c++) {
          t[0][c] += X[c] * ds[pts[p].d0][a];
          t[1][c] += X[c] * ds[pts[p].d1][a];
        }
      }
      const double cr[3] = {t[0][1] * t[1][2] - t[0][2] * t[1][1], t[0][2] * t[1][0] - t[0][0] * t[1][2],
                            t[0][0] * t[1][1] - t[0][1] * t[1][0]};
      out.w[(size_t)e * 32 + p] = pts[p].qw * std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    }
  }
  return out;
}

}  // namespace ancf
}  // namespace tlfea
