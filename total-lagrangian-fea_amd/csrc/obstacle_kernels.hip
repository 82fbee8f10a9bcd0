// obstacle_kernels.hip -- implicit contact of T10 surface nodes with rigid half-spaces, spheres and signed-distance
// fields (DESIGN 3e, 3e'').
//
//   obstacle_grad_kernel<F>    (F: the list holds field obstacles) one thread per surface node: evaluates every obstacle of the list (kernel argument),
//                              adds grad Phi to g and keeps the node's force, its 3x3 Hessian block and its per-obstacle
//                              share for the Hessian launch and the resultants
//   obstacle_hessian_kernel    one thread per surface node: h x the block into the node's own diagonal block of H
//   obstacle_resultant_kernel  one block per obstacle: fixed-order sum of the per-node shares
//
// The model of one (node, obstacle) pair is obstacle_point.h's, shared with the ANCF sample points (DESIGN 3e').
// No atomics: every node owns its entries, so the results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <cmath>

#include "obstacle_point.h"
#include "tlfea_internal.h"

namespace tlfea {
namespace {

constexpr int kBlock = 256;

template <bool kFields>
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
      bool fric;
      obstacle_point_terms<kFields>(o, wk, q, q0, h, fj, B, act, fric);
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
  if (L.has_fields())
    hipLaunchKernelGGL(obstacle_grad_kernel<true>, dim3(blocks(n_surf)), dim3(kBlock), 0, s, n_surf, node, w, L, x, y, z,
                       xp, yp, zp, h, fixed_slot, g, f, blk, fk);
  else
    hipLaunchKernelGGL(obstacle_grad_kernel<false>, dim3(blocks(n_surf)), dim3(kBlock), 0, s, n_surf, node, w, L, x, y, z,
                       xp, yp, zp, h, fixed_slot, g, f, blk, fk);
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
