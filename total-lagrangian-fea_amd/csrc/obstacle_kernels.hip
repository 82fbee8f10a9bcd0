// obstacle_kernels.hip -- implicit contact of T10 surface nodes with rigid half-spaces and spheres.
//
//   obstacle_grad_kernel       one thread per surface node: evaluates every obstacle of the list (kernel argument),
//                              adds grad Phi to g and keeps the node's force, its 3x3 Hessian block and its per-obstacle
//                              share for the Hessian launch and the resultants
//   obstacle_hessian_kernel    one thread per surface node: h x the block into the node's own diagonal block of H
//   obstacle_resultant_kernel  one block per obstacle: fixed-order sum of the per-node shares
//
// Model, per surface node of weight w (surface area share) and obstacle of stiffness kappa (Pa/m):
//   normal    Phi_n = 1/2 kappa w <-d>^2, d the signed distance; Hessian kappa w n n^T (exact for a half-space, the
//             Gauss-Newton form for a sphere: the curvature term is negative in contact and is dropped)
//   friction  Phi_t = mu lam0 f0(|u|), lam0 = kappa w <-d(x_prev)>, u = P_t (x - x_prev - h v_o), P_t and lam0 from the
//             start-of-step positions; f1 = f0' = 2y/eps - y^2/eps^2 below eps = eps_v h, 1 above.
// No atomics: every node owns its entries, so the results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tlfea_internal.h"

namespace tlfea {
namespace {

constexpr int kBlock = 256;

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

__global__ __launch_bounds__(kBlock) void obstacle_grad_kernel(int n_surf, const int* __restrict__ node,
                                                               const double* __restrict__ w, ObstacleList L,
                                                               const double* __restrict__ x, const double* __restrict__ y,
                                                               const double* __restrict__ z, const double* __restrict__ xp,
                                                               const double* __restrict__ yp, const double* __restrict__ zp,
                                                               double h, const int* __restrict__ fixed_slot,
                                                               double* __restrict__ g, double* __restrict__ fout,
                                                               double* __restrict__ blk, double* __restrict__ fk) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_surf) return;
  const int i = node[k];
  const bool pinned = fixed_slot && fixed_slot[i] >= 0;
  const double wk = w[k];
  const double q[3] = {x[i], y[i], z[i]};
  const double q0[3] = {xp[i], yp[i], zp[i]};
  double f[3] = {0.0, 0.0, 0.0}, B[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < L.n; j++) {
    const ObstacleDev& o = L.o[j];
    double fj[3] = {0.0, 0.0, 0.0}, act = 0.0;
    if (!pinned) {
      double nrm[3];
      const double d = obstacle_distance(o, q, nrm);
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
    }
    double* r = fk + ((size_t)j * n_surf + k) * 4;
    r[0] = fj[0];
    r[1] = fj[1];
    r[2] = fj[2];
    r[3] = act;
    f[0] += fj[0];
    f[1] += fj[1];
    f[2] += fj[2];
  }
  if (g) {
    g[3 * i + 0] -= f[0];
    g[3 * i + 1] -= f[1];
    g[3 * i + 2] -= f[2];
  }
  for (int c = 0; c < 3; c++) fout[3 * (size_t)k + c] = f[c];
  for (int c = 0; c < 6; c++) blk[6 * (size_t)k + c] = B[c];
}

// diagonal block of node i in H: row d at 9 off[i] + d * 3 deg, column 3 diagpos[i] (assemble_rows_kernel's layout)
__global__ __launch_bounds__(kBlock) void obstacle_hessian_kernel(int n_surf, const int* __restrict__ node,
                                                                  const int* __restrict__ off,
                                                                  const int* __restrict__ diagpos,
                                                                  const double* __restrict__ blk, double h,
                                                                  double* __restrict__ H) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_surf) return;
  const int i = node[k];
  const int o = off[i], deg = off[i + 1] - o;
  double* D = H + (size_t)9 * o + 3 * diagpos[i];
  const double* b = blk + 6 * (size_t)k;
  const double B[3][3] = {{b[0], b[3], b[4]}, {b[3], b[1], b[5]}, {b[4], b[5], b[2]}};
  for (int d = 0; d < 3; d++)
    for (int e = 0; e < 3; e++) D[(size_t)d * 3 * deg + e] += h * B[d][e];
}

__global__ __launch_bounds__(kBlock) void obstacle_resultant_kernel(int n_surf, const double* __restrict__ fk,
                                                                    double* __restrict__ out) {
  __shared__ double acc[4][kBlock];
  const int j = blockIdx.x, t = threadIdx.x;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = t; k < n_surf; k += kBlock) {
    const double* r = fk + ((size_t)j * n_surf + k) * 4;
    for (int c = 0; c < 4; c++) a[c] += r[c];
  }
  for (int c = 0; c < 4; c++) acc[c][t] = a[c];
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int c = 0; c < 4; c++) acc[c][t] += acc[c][t + s];
    __syncthreads();
  }
  if (t < 4) out[4 * j + t] = acc[t][0];
}

inline int blocks(int n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

void launch_obstacle_grad(hipStream_t s, int n_surf, const int* node, const double* w, const ObstacleList& L,
                          const double* x, const double* y, const double* z, const double* xp, const double* yp,
                          const double* zp, double h, const int* fixed_slot, double* g, double* f, double* blk,
                          double* fk) {
  if (n_surf <= 0) return;
  hipLaunchKernelGGL(obstacle_grad_kernel, dim3(blocks(n_surf)), dim3(kBlock), 0, s, n_surf, node, w, L, x, y, z, xp, yp,
                     zp, h, fixed_slot, g, f, blk, fk);
}

void launch_obstacle_hessian(hipStream_t s, int n_surf, const int* node, const int* off, const int* diagpos,
                             const double* blk, double h, double* H) {
  if (n_surf <= 0) return;
  hipLaunchKernelGGL(obstacle_hessian_kernel, dim3(blocks(n_surf)), dim3(kBlock), 0, s, n_surf, node, off, diagpos, blk,
                     h, H);
}

void launch_obstacle_resultant(hipStream_t s, int n_surf, int n_obs, const double* fk, double* out) {
  if (n_obs <= 0) return;
  hipLaunchKernelGGL(obstacle_resultant_kernel, dim3(n_obs), dim3(kBlock), 0, s, n_surf, fk, out);
}

}  // namespace tlfea
