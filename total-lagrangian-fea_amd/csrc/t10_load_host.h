// t10_load_host.h -- host side of the surface loads on the boundary faces of a T10 mesh (DESIGN 3h'): the boundary faces
// with their nodes ordered outward, the 6-point triangle rule and the traction weights of a face.  Included by
// data_handle.h (the handle keeps the faces) for loads_api.hip.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <vector>

#include "obstacle_host.h"

namespace tlfea {
namespace t10load {

// The 6-point rule of degree 4 on the unit triangle (xi, eta, weight; the weights sum to 1/2).  load_kernels.hip holds the
// same numbers.
constexpr double kTriRule[6][3] = {
    {0.44594849091596488632, 0.44594849091596488632, 0.11169079483900573285},
    {0.10810301816807022736, 0.44594849091596488632, 0.11169079483900573285},
    {0.44594849091596488632, 0.10810301816807022736, 0.11169079483900573285},
    {0.09157621350977074346, 0.09157621350977074346, 0.05497587182766093382},
    {0.81684757298045851308, 0.09157621350977074346, 0.05497587182766093382},
    {0.09157621350977074346, 0.81684757298045851308, 0.05497587182766093382}};

// quadratic triangle: corners 0 1 2, mid-edge nodes 01 12 02 (the order of kFace)
inline void tri6(double xi, double eta, double N[6], double dx[6], double de[6]) {
  const double l0 = 1.0 - xi - eta;
  N[0] = l0 * (2 * l0 - 1), N[1] = xi * (2 * xi - 1), N[2] = eta * (2 * eta - 1);
  N[3] = 4 * l0 * xi, N[4] = 4 * xi * eta, N[5] = 4 * l0 * eta;
  dx[0] = -(4 * l0 - 1), dx[1] = 4 * xi - 1, dx[2] = 0.0, dx[3] = 4 * (l0 - xi), dx[4] = 4 * eta, dx[5] = -4 * eta;
  de[0] = -(4 * l0 - 1), de[1] = 0.0, de[2] = 4 * eta - 1, de[3] = -4 * xi, de[4] = 4 * xi, de[5] = 4 * (l0 - eta);
}

struct BoundaryFaces {
  std::vector<int> elem, local_face, nodes;  // [F], [F], [F][6]
  int count() const { return (int)elem.size(); }
};

// Ascending (element, local face).  The six nodes are reordered once (two corners and their mid-edge nodes swapped) so
// that X_xi x X_eta points away from the tet's fourth vertex in the reference configuration.  conn_cm: [10][E],
// X0: x | y | z.
inline BoundaryFaces boundary_faces(int E, int N, const std::vector<int>& conn_cm, const std::vector<double>& X0) {
  std::vector<std::array<int, 2>> ef = t10_boundary_face_search(E, conn_cm);
  std::sort(ef.begin(), ef.end());
  BoundaryFaces out;
  for (const std::array<int, 2>& r : ef) {
    const int e = r[0], f = r[1];
    int nd[6];
    for (int t = 0; t < 6; t++) nd[t] = conn_cm[(size_t)kFace[f][t] * E + e];
    const int fourth = conn_cm[(size_t)(6 - kFace[f][0] - kFace[f][1] - kFace[f][2]) * E + e];
    double u[3], v[3], w[3];
    for (int c = 0; c < 3; c++) {
      u[c] = X0[(size_t)c * N + nd[1]] - X0[(size_t)c * N + nd[0]];
      v[c] = X0[(size_t)c * N + nd[2]] - X0[(size_t)c * N + nd[0]];
      w[c] = X0[(size_t)c * N + fourth] - X0[(size_t)c * N + nd[0]];
    }
    const double cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    if (cr[0] * w[0] + cr[1] * w[1] + cr[2] * w[2] > 0.0) {
      std::swap(nd[1], nd[2]);
      std::swap(nd[3], nd[5]);
    }
    out.elem.push_back(e);
    out.local_face.push_back(f);
    out.nodes.insert(out.nodes.end(), nd, nd + 6);
  }
  return out;
}

// w_a = sum_q w_q N_a(q) |X_xi x X_eta|(q), points in rule order
inline void traction_weights(const int nd[6], int N, const std::vector<double>& X0, double w[6]) {
  for (int a = 0; a < 6; a++) w[a] = 0.0;
  for (int q = 0; q < 6; q++) {
    double Nq[6], dx[6], de[6];
    tri6(kTriRule[q][0], kTriRule[q][1], Nq, dx, de);
    double t0[3] = {0, 0, 0}, t1[3] = {0, 0, 0};
    for (int a = 0; a < 6; a++)
      for (int c = 0; c < 3; c++) {
        t0[c] += dx[a] * X0[(size_t)c * N + nd[a]];
        t1[c] += de[a] * X0[(size_t)c * N + nd[a]];
      }
    const double cr[3] = {t0[1] * t1[2] - t0[2] * t1[1], t0[2] * t1[0] - t0[0] * t1[2], t0[0] * t1[1] - t0[1] * t1[0]};
    const double dA = kTriRule[q][2] * std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    for (int a = 0; a < 6; a++) w[a] += Nq[a] * dA;
  }
}

}  // namespace t10load
}  // namespace tlfea
