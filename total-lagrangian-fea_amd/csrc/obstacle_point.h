// obstacle_point.h -- the per-point physics of the rigid obstacles, shared by the T10 node kernel
// (obstacle_kernels.hip) and the ANCF sample-point kernel (ancf_obstacle_kernels.hip, DESIGN 3e').  Device code only.
//
// Model, per point of weight w (surface area share) and obstacle of stiffness kappa (Pa/m):
//   normal    Phi_n = 1/2 kappa w <-d>^2, d the signed distance; Hessian kappa w n n^T (exact for a half-space, the
//             Gauss-Newton form for a sphere: the curvature term is negative in contact and is dropped)
//   friction  Phi_t = mu lam0 f0(|u|), lam0 = kappa w <-d(x_prev)>, u = P_t (x - x_prev - h v_o), P_t and lam0 from the
//             start-of-step positions; f1 = f0' = 2y/eps - y^2/eps^2 below eps = eps_v h, 1 above.
// A field obstacle (kind 2, DESIGN 3e'') puts the interpolated gap phi in the place of d and its gradient G (not
// normalised) in the place of n: force kappa w <-phi> G, block kappa w G G^T; friction from n0 = G(x_prev) / |G(x_prev)| and
// lam0 = kappa w <-phi(x_prev)> |G(x_prev)|.  Outside the field's coverage it contributes exactly nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "tlfea_internal.h"

namespace tlfea {

// signed distance and outward unit normal of obstacle o at point q
__device__ __forceinline__ double obstacle_distance(const ObstacleDev& o, const double q[3], double nrm[3]) {
  if (o.kind == kHalfSpace) {
    nrm[0] = o.n[0];
    nrm[1] = o.n[1];
    nrm[2] = o.n[2];
    return o.n[0] * (q[0] - o.p[0]) + o.n[1] * (q[1] - o.p[1]) + o.n[2] * (q[2] - o.p[2]);
  }
  const double r[3] = {q[0] - o.p[0], q[1] - o.p[1], q[2] - o.p[2]};
  const double rl = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (rl > 0.0) {
    nrm[0] = r[0] / rl;
    nrm[1] = r[1] / rl;
    nrm[2] = r[2] / rl;
  } else {  // at the centre: any direction is a closest one
    nrm[0] = 0.0;
    nrm[1] = 0.0;
    nrm[2] = 1.0;
  }
  return rl - o.radius;
}

// block storage: xx yy zz xy xz yz
__device__ __forceinline__ void add_outer(double B[6], double c, const double a[3], const double b[3]) {
  B[0] += c * a[0] * b[0];
  B[1] += c * a[1] * b[1];
  B[2] += c * a[2] * b[2];
  B[3] += c * a[0] * b[1];
  B[4] += c * a[0] * b[2];
  B[5] += c * a[1] * b[2];
}

// The regularised friction term of one (point, obstacle) pair: lam0 the start-of-step normal force, n0 the
// start-of-step unit normal.  Adds its force to fj and its block to B.
__device__ __forceinline__ void obstacle_friction_terms(const ObstacleDev& o, double lam0, const double n0[3],
                                                        const double q[3], const double q0[3], double h, double fj[3],
                                                        double B[6]) {
  double u[3];
  for (int c = 0; c < 3; c++) u[c] = q[c] - q0[c] - h * o.vel[c];
  const double un = n0[0] * u[0] + n0[1] * u[1] + n0[2] * u[2];
  for (int c = 0; c < 3; c++) u[c] -= un * n0[c];
  const double yl = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double eps = o.eps_v * h;
  // f1y = f1(y) / y and f1p = f1'(y); both tend to 2/eps at y = 0
  double f1y, f1p;
  if (yl >= eps) {
    f1y = 1.0 / yl;
    f1p = 0.0;
  } else {
    f1y = 2.0 / eps - yl / (eps * eps);
    f1p = 2.0 / eps - 2.0 * yl / (eps * eps);
  }
  const double c0 = o.mu * lam0;
  for (int c = 0; c < 3; c++) fj[c] -= c0 * f1y * u[c];
  // mu lam0 (f1y P_t + (f1p - f1y) u u^T / y^2): symmetric PSD on both branches
  const double id[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int c = 0; c < 3; c++) add_outer(B, c0 * f1y, id[c], id[c]);
  add_outer(B, -c0 * f1y, n0, n0);
  if (yl > 0.0) add_outer(B, c0 * (f1p - f1y) / (yl * yl), u, u);
}

// Gap phi and world gradient G of field obstacle o at the world point q: the uniform quadratic B-spline over the 27
// samples around the nearest one, summed z, y, x outermost to innermost.  False (and nothing written) outside coverage,
// 0.5 <= g_a <= n_a - 1.5 on every axis; a NaN coordinate is outside.
__device__ __forceinline__ bool field_eval(const ObstacleDev& o, const double q[3], double& phi, double G[3]) {
  const FieldDev& F = *o.fld;
  const double r[3] = {q[0] - o.p[0], q[1] - o.p[1], q[2] - o.p[2]};
  const int n[3] = {F.nx, F.ny, F.nz};
  int i[3];
  double w[3][3], dw[3][3];
  for (int a = 0; a < 3; a++) {
    const double sa = F.rot[a] * r[0] + F.rot[3 + a] * r[1] + F.rot[6 + a] * r[2];  // rot^T r
    const double ga = (sa - F.origin[a]) / F.spacing;
    if (!(ga >= 0.5 && ga <= (double)n[a] - 1.5)) return false;
    int ia = (int)floor(ga + 0.5);
    ia = ia < 1 ? 1 : (ia > n[a] - 2 ? n[a] - 2 : ia);
    const double t = ga - (double)ia;
    i[a] = ia;
    w[a][0] = 0.5 * (0.5 - t) * (0.5 - t);
    w[a][1] = 0.75 - t * t;
    w[a][2] = 0.5 * (0.5 + t) * (0.5 + t);
    dw[a][0] = -(0.5 - t);
    dw[a][1] = -2.0 * t;
    dw[a][2] = 0.5 + t;
  }
  double f = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
  for (int c = 0; c < 3; c++)
    for (int b = 0; b < 3; b++) {
      const double* row = F.V + ((size_t)(i[2] - 1 + c) * n[1] + (size_t)(i[1] - 1 + b)) * n[0] + (size_t)(i[0] - 1);
      const double v0 = row[0], v1 = row[1], v2 = row[2];
      const double rx = w[0][0] * v0 + w[0][1] * v1 + w[0][2] * v2;
      const double rdx = dw[0][0] * v0 + dw[0][1] * v1 + dw[0][2] * v2;
      f += w[2][c] * w[1][b] * rx;
      gx += w[2][c] * w[1][b] * rdx;
      gy += w[2][c] * dw[1][b] * rx;
      gz += dw[2][c] * w[1][b] * rx;
    }
  gx /= F.spacing;
  gy /= F.spacing;
  gz /= F.spacing;
  phi = f;
  for (int a = 0; a < 3; a++) G[a] = F.rot[3 * a] * gx + F.rot[3 * a + 1] * gy + F.rot[3 * a + 2] * gz;
  return true;
}

// obstacle_point_terms of a field obstacle; returns phi at q, +inf where the field does not cover q
__device__ __forceinline__ double field_point_terms(const ObstacleDev& o, double wk, const double q[3],
                                                    const double q0[3], double h, double fj[3], double B[6], double& act,
                                                    bool& fric) {
  double phi = INFINITY, G[3];
  fric = false;
  if (field_eval(o, q, phi, G) && phi < 0.0) {
    const double lam = o.kappa * wk * (-phi);
    for (int c = 0; c < 3; c++) fj[c] += lam * G[c];
    add_outer(B, o.kappa * wk, G, G);
    act = 1.0;
  }
  if (o.mu > 0.0) {
    double phi0, G0[3];
    if (field_eval(o, q0, phi0, G0) && phi0 < 0.0) {
      const double gl = sqrt(G0[0] * G0[0] + G0[1] * G0[1] + G0[2] * G0[2]);
      if (gl > 0.0) {
        fric = true;
        const double n0[3] = {G0[0] / gl, G0[1] / gl, G0[2] / gl};
        const double lam0 = o.kappa * wk * (-phi0) * gl;
        obstacle_friction_terms(o, lam0, n0, q, q0, h, fj, B);
      }
    }
  }
  return phi;
}

// One obstacle at one point of weight wk: q the current position, q0 the start-of-step one.  Adds the obstacle's force
// -grad Phi to fj and its Hessian block to B, sets act = 1 if the point penetrates now and fric if the friction term is
// active (the point penetrated at the start of the step).  Returns the signed distance at q.
// kFields: the list may hold field obstacles.  The launches pick the instantiation by the list, so that a list of
// analytic obstacles alone runs the code -- and keeps the registers -- it had before fields existed (DESIGN 3e'').
template <bool kFields>
__device__ __forceinline__ double obstacle_point_terms(const ObstacleDev& o, double wk, const double q[3],
                                                       const double q0[3], double h, double fj[3], double B[6],
                                                       double& act, bool& fric) {
  if (kFields && o.kind == kField) return field_point_terms(o, wk, q, q0, h, fj, B, act, fric);
  double nrm[3];
  const double d = obstacle_distance(o, q, nrm);
  fric = false;
  if (d < 0.0) {
    const double lam = o.kappa * wk * (-d);
    for (int c = 0; c < 3; c++) fj[c] += lam * nrm[c];
    add_outer(B, o.kappa * wk, nrm, nrm);
    act = 1.0;
  }
  if (o.mu > 0.0) {
    double n0[3];
    const double d0 = obstacle_distance(o, q0, n0);
    if (d0 < 0.0) {
      fric = true;
      const double lam0 = o.kappa * wk * (-d0);
      obstacle_friction_terms(o, lam0, n0, q, q0, h, fj, B);
    }
  }
  return d;
}

}  // namespace tlfea
