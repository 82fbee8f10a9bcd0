// ancf_load_host.h -- host side of the follower pressure on the ANCF kinds: the Gauss points of a face and,
// per distinct (L, W, H), the shape values and the two tangential shape derivatives at them.  The dead traction needs no
// table of its own: it uses the sample points and weights of ancf_obstacle_host.h.  Included by loads_api.hip only.
#pragma once
#include <array>
#include <map>
#include <vector>

#include "ancf_obstacle_host.h"

namespace tlfea {
namespace ancf {

inline int load_faces(int S) { return S == 16 ? 2 : 4; }
inline int load_points(int S) { return S == 16 ? 25 : 10; }
// sign s with (outward normal) dA = s (r_d0 x r_d1) d(d0) d(d1) on face f, d0 and d1 the face's two directions in the
// order of SamplePoint (shell: xi, eta; beam faces 0, 1: xi, zeta; beam faces 2, 3: xi, eta)
inline double load_face_sign(int S, int f) {
  if (S == 16) return f ? 1.0 : -1.0;
  return (f == 0 || f == 3) ? 1.0 : -1.0;
}

// On a shell face the integrand S_a (r_xi x r_eta) has degree up to 8 in xi and in eta (S_a 3, the cross product 2 + 3),
// one more than the 4-point rule integrates: 5 Gauss points each way.  On a beam face it has degree 6 along xi (3 + 2 + 1)
// and 2 across (S_a and the cross product are linear there): 5 x 2 points, the same rule along xi as the shell's.
// Shell: q = ixi * 5 + ieta.  Beam: q = ixi * 2 + k.
inline std::vector<SamplePoint> pressure_points(int S, int f) {
  const double g5[5] = {-0.9061798459386640, -0.5384693101056831, 0.0, 0.5384693101056831, 0.9061798459386640};
  const double w5[5] = {0.2369268850561891, 0.4786286704993665, 0.5688888888888889, 0.4786286704993665,
                        0.2369268850561891};
  const double g2[2] = {-0.5773502691896257, 0.5773502691896257};
  const double sgn = (f & 1) ? 1.0 : -1.0;
  std::vector<SamplePoint> pts;
  for (int i = 0; i < 5; i++) {
    if (S == 16) {
      for (int j = 0; j < 5; j++) pts.push_back({g5[i], g5[j], sgn, w5[i] * w5[j], 0, 1});
    } else {
      for (int k = 0; k < 2; k++)
        pts.push_back(f < 2 ? SamplePoint{g5[i], sgn, g2[k], w5[i], 0, 2} : SamplePoint{g5[i], g2[k], sgn, w5[i], 0, 1});
    }
  }
  return pts;
}

struct PressureSetup {
  std::vector<int> cls;     // [E]
  std::vector<double> tab;  // [n_class][nface][P][3][S]
  std::vector<double> qw;   // [P]
};

inline PressureSetup pressure_setup(int S, int E, const std::vector<double>& Lv, const std::vector<double>& Wv,
                                    const std::vector<double>& Hv, const std::vector<double>& Binv) {
  const int NF = load_faces(S), P = load_points(S);
  const Basis B = basis(S);
  PressureSetup out;
  out.cls.resize(E);
  for (const SamplePoint& p : pressure_points(S, 0)) out.qw.push_back(p.qw);
  std::map<std::array<double, 3>, int> seen;
  for (int e = 0; e < E; e++) {
    const std::array<double, 3> key = {Lv[e], Wv[e], Hv[e]};
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(key, (int)seen.size()).first;
      const double* Bi = &Binv[(size_t)e * S * S];
      out.tab.resize(seen.size() * NF * P * 3 * S);
      double* tab = &out.tab[(size_t)it->second * NF * P * 3 * S];
      for (int f = 0; f < NF; f++) {
        const std::vector<SamplePoint> pts = pressure_points(S, f);
        for (int q = 0; q < P; q++) {
          double b[16], ds[3][16];
          double* row = tab + ((size_t)f * P + q) * 3 * S;
          eval(B, Lv[e] * pts[q].xi / 2, Wv[e] * pts[q].eta / 2, Hv[e] * pts[q].zeta / 2, 0, b);
          ds_dxi(S, Bi, Lv[e], Wv[e], Hv[e], pts[q].xi, pts[q].eta, pts[q].zeta, ds);
          for (int i = 0; i < S; i++) {
            double a = 0.0;
            for (int j = 0; j < S; j++) a += Bi[(size_t)j * S + i] * b[j];
            row[i] = a;
            row[S + i] = ds[pts[q].d0][i];
            row[2 * S + i] = ds[pts[q].d1][i];
          }
        }
      }
    }
    out.cls[e] = it->second;
  }
  return out;
}

}  // namespace ancf
}  // namespace tlfea
