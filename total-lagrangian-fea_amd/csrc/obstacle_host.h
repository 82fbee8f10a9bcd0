// obstacle_host.h -- host side of the rigid obstacles: the surface weights of a T10 mesh and the argument
// checks of one obstacle.  Included by obstacle_api.hip and t10_load_host.h.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/tlfea_c.h"
#include "tlfea_internal.h"

namespace tlfea {

// faces of the T10 tet: corners, then the mid-edge nodes of edges 01 -> 4, 12 -> 5, 02 -> 6, 03 -> 7, 13 -> 8, 23 -> 9
constexpr int kFace[4][6] = {{0, 1, 2, 4, 5, 6}, {0, 1, 3, 4, 8, 7}, {0, 2, 3, 6, 9, 7}, {1, 2, 3, 5, 9, 8}};

// The boundary faces of a T10 mesh as (element, local face): a boundary face is a 6-node triangle that belongs to exactly
// one tet, found by its sorted corner triple.  They come in ascending order of that triple.  conn_cm: [10][E].
inline std::vector<std::array<int, 2>> t10_boundary_face_search(int E, const std::vector<int>& conn_cm) {
  struct Rec {
    std::array<int, 3> key;
    int e, f;
  };
  std::vector<Rec> faces;
  faces.reserve((size_t)4 * E);
  for (int e = 0; e < E; e++)
    for (int f = 0; f < 4; f++) {
      std::array<int, 3> k = {conn_cm[(size_t)kFace[f][0] * E + e], conn_cm[(size_t)kFace[f][1] * E + e],
                              conn_cm[(size_t)kFace[f][2] * E + e]};
      std::sort(k.begin(), k.end());
      faces.push_back({k, e, f});
    }
  std::sort(faces.begin(), faces.end(), [](const Rec& a, const Rec& b) {
    return a.key != b.key ? a.key < b.key : (a.e != b.e ? a.e < b.e : a.f < b.f);
  });
  std::vector<std::array<int, 2>> out;
  for (size_t a = 0; a < faces.size();) {
    size_t b = a + 1;
    while (b < faces.size() && faces[b].key == faces[a].key) b++;
    if (b - a == 1) out.push_back({faces[a].e, faces[a].f});
    a = b;
  }
  return out;
}

// Surface weight of every node: each of the six nodes of a boundary face gets A_f / 6, A_f the area of its corner
// triangle in the reference configuration.  The weights sum to the surface area; interior nodes get 0.  conn_cm: [10][E]
// (the setup layout), X0: x | y | z.
inline std::vector<double> t10_surface_weights(int E, int N, const std::vector<int>& conn_cm, const std::vector<double>& X0) {
  std::vector<double> w((size_t)N, 0.0);
  for (const std::array<int, 2>& ef : t10_boundary_face_search(E, conn_cm)) {
    const int e = ef[0], f = ef[1];
    int nd[6];
    for (int t = 0; t < 6; t++) nd[t] = conn_cm[(size_t)kFace[f][t] * E + e];
    double p[3][3];
    for (int c = 0; c < 3; c++)
      for (int t = 0; t < 3; t++) p[c][t] = X0[(size_t)t * N + nd[c]];
    const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double v[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double A = 0.5 * std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    for (int t = 0; t < 6; t++) w[nd[t]] += A / 6.0;
  }
  return w;
}

// empty string: the obstacle is valid; otherwise what is wrong with it
inline std::string obstacle_check(const tlfea_obstacle& o) {
  if (o.kind != kHalfSpace && o.kind != kSphere)
    return "unknown kind " + std::to_string(o.kind) + " (0 half-space, 1 sphere)";
  for (double v : {o.p[0], o.p[1], o.p[2], o.n[0], o.n[1], o.n[2], o.radius, o.vel[0], o.vel[1], o.vel[2], o.stiffness,
                   o.friction, o.eps_v})
    if (!std::isfinite(v)) return "non-finite parameter";
  if (!(o.stiffness > 0.0)) return "stiffness must be > 0 (Pa/m)";
  if (!(o.friction >= 0.0)) return "friction must be >= 0";
  if (!(o.eps_v > 0.0)) return "eps_v must be > 0 (m/s)";
  if (o.kind == kHalfSpace) {
    const double nn = std::sqrt(o.n[0] * o.n[0] + o.n[1] * o.n[1] + o.n[2] * o.n[2]);
    if (!(std::fabs(nn - 1.0) <= 1e-12)) return "the half-space normal must have unit length (to 1e-12)";
  } else if (!(o.radius > 0.0)) {
    return "sphere radius must be > 0";
  }
  return "";
}

inline ObstacleDev obstacle_dev(const tlfea_obstacle& o) {
  ObstacleDev d;
  d.kind = o.kind;
  for (int c = 0; c < 3; c++) {
    d.p[c] = o.p[c];
    d.n[c] = o.kind == kHalfSpace ? o.n[c] : 0.0;
    d.vel[c] = o.vel[c];
  }
  d.radius = o.kind == kSphere ? o.radius : 0.0;
  d.kappa = o.stiffness;
  d.mu = o.friction;
  d.eps_v = o.eps_v;
  d.fld = nullptr;
  return d;
}

}  // namespace tlfea
