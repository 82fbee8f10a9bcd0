// obstacle_point.h -- the per-point physics of the rigid obstacles, shared by the T10 node kernel
// (obstacle_kernels.hip) and the ANCF sample-point kernel (ancf_obstacle_kernels.hip, DESIGN 3e').  Device code only.
//
// Model, per point of weight w (surface area share) and obstacle of stiffness kappa (Pa/m):
//   normal    Phi_n = 1/2 kappa w <-d>^2, d the signed distance; Hessian kappa w n n^T (exact for a half-space, the
//             Gauss-Newton form for a sphere: the curvature term is negative in contact and is dropped)
//   friction  Phi_t = mu lam0 f0(|u|), lam0 = kappa w <-d(x_prev)>, u = P_t (x - x_prev - h v_o), P_t and lam0 from the
//             start-of-step positions; f1 = f0' = 2y/eps - y^2/eps^2 below eps = eps_v h, 1 above.
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

// One obstacle at one point of weight wk: q the current position, q0 the start-of-step one.  Adds the obstacle's force
// -grad Phi to fj and its Hessian block to B, sets act = 1 if the point penetrates now and fric if the friction term is
// active (the point penetrated at the start of the step).  Returns the signed distance at q.
__device__ __forceinline__ double obstacle_point_terms(const ObstacleDev& o, double wk, const double q[3],
                                                       const double q0[3], double h, double fj[3], double B[6],
                                                       double& act, bool& fric) {
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
  }
  return d;
}

}  // namespace tlfea
