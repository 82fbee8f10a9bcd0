// field_obstacle_host.h -- host side of the field obstacles (DESIGN 3e''): the argument checks of one field and of a
// triangle surface handed to the builder.  Included by obstacle_api.hip only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/tlfea_c.h"
#include "tlfea_internal.h"

namespace tlfea {

constexpr long long kMaxFieldSamples = 1ll << 27;

// the parameters of a field without its samples; empty string: valid
inline std::string field_params_check(const tlfea_field_obstacle& o) {
  if (o.nx < 5 || o.ny < 5 || o.nz < 5)
    return "every axis needs at least 5 samples, got " + std::to_string(o.nx) + " x " + std::to_string(o.ny) + " x " +
           std::to_string(o.nz);
  if ((long long)o.nx * o.ny * o.nz > kMaxFieldSamples) return "more than 2^27 samples";
  for (double v : {o.origin[0], o.origin[1], o.origin[2], o.spacing, o.pos[0], o.pos[1], o.pos[2], o.vel[0], o.vel[1],
                   o.vel[2], o.stiffness, o.friction, o.eps_v})
    if (!std::isfinite(v)) return "non-finite parameter";
  for (double v : o.rot)
    if (!std::isfinite(v)) return "non-finite parameter";
  if (!(o.spacing > 0.0)) return "spacing must be > 0";
  if (!(o.stiffness > 0.0)) return "stiffness must be > 0 (Pa/m)";
  if (!(o.friction >= 0.0)) return "friction must be >= 0";
  if (!(o.eps_v > 0.0)) return "eps_v must be > 0 (m/s)";
  const double* R = o.rot;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      const double d = R[3 * a] * R[3 * b] + R[3 * a + 1] * R[3 * b + 1] + R[3 * a + 2] * R[3 * b + 2];
      if (!(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-12)) return "the rotation must be orthonormal (to 1e-12)";
    }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                     R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (!(det > 0.0)) return "the rotation must have determinant +1";
  return "";
}

// the closed-shape rule: every sample finite, the two outermost layers of each axis > 0
inline std::string field_values_check(const tlfea_field_obstacle& o, const double* V) {
  const int n[3] = {o.nx, o.ny, o.nz};
  for (int iz = 0; iz < n[2]; iz++)
    for (int iy = 0; iy < n[1]; iy++) {
      const bool rim_yz = iz < 2 || iz >= n[2] - 2 || iy < 2 || iy >= n[1] - 2;
      const double* row = V + ((size_t)iz * n[1] + iy) * n[0];
      for (int ix = 0; ix < n[0]; ix++) {
        if (!std::isfinite(row[ix])) return "non-finite sample";
        if ((rim_yz || ix < 2 || ix >= n[0] - 2) && !(row[ix] > 0.0))
          return "a sample in the two outermost layers is not > 0 (the body must lie well inside its grid)";
      }
    }
  return "";
}

// a closed, consistently oriented surface without degenerate triangles: every directed edge once, its reverse once
inline std::string surface_check(const double* verts, int n_verts, const int* tris, int n_tris) {
  if (n_verts < 4 || n_tris < 4) return "a closed surface needs at least 4 vertices and 4 triangles";
  for (int i = 0; i < 3 * n_verts; i++)
    if (!std::isfinite(verts[i])) return "non-finite vertex";
  std::vector<std::uint64_t> edges;
  edges.reserve((size_t)3 * n_tris);
  for (int t = 0; t < n_tris; t++) {
    const int* v = tris + 3 * t;
    for (int c = 0; c < 3; c++)
      if (v[c] < 0 || v[c] >= n_verts)
        return "triangle " + std::to_string(t) + ": vertex index " + std::to_string(v[c]) + " out of range";
    const double *a = verts + 3 * v[0], *b = verts + 3 * v[1], *c = verts + 3 * v[2];
    const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double cr[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    if (!(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2] > 0.0)) return "triangle " + std::to_string(t) + " has zero area";
    for (int c2 = 0; c2 < 3; c2++)
      edges.push_back(((std::uint64_t)(std::uint32_t)v[c2] << 32) | (std::uint32_t)v[(c2 + 1) % 3]);
  }
  std::sort(edges.begin(), edges.end());
  for (size_t i = 0; i + 1 < edges.size(); i++)
    if (edges[i] == edges[i + 1]) return "the surface is not consistently oriented (a directed edge occurs twice)";
  for (std::uint64_t e : edges)
    if (!std::binary_search(edges.begin(), edges.end(), (e << 32) | (e >> 32)))
      return "the surface is open (an edge has no opposite)";
  return "";
}

inline FieldDev field_dev(const tlfea_field_obstacle& o, const double* d_V) {
  FieldDev f;
  f.nx = o.nx;
  f.ny = o.ny;
  f.nz = o.nz;
  for (int c = 0; c < 3; c++) f.origin[c] = o.origin[c];
  f.spacing = o.spacing;
  for (int c = 0; c < 9; c++) f.rot[c] = o.rot[c];
  f.V = d_V;
  return f;
}

inline ObstacleDev field_obstacle_dev(const tlfea_field_obstacle& o, const FieldDev* d_fld) {
  ObstacleDev d;
  d.kind = kField;
  for (int c = 0; c < 3; c++) {
    d.p[c] = o.pos[c];
    d.n[c] = 0.0;
    d.vel[c] = o.vel[c];
  }
  d.radius = 0.0;
  d.kappa = o.stiffness;
  d.mu = o.friction;
  d.eps_v = o.eps_v;
  d.fld = d_fld;
  return d;
}

}  // namespace tlfea
