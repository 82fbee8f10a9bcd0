// ancf_obstacle_kernels.hip -- implicit contact of ANCF-3243 beams and ANCF-3443 shells with rigid half-spaces,
// spheres and signed-distance fields (DESIGN 3e', 3e'').  Contact is evaluated at 32 sample points on the faces of every element and spread to the
// element's S coefficient vectors through the shape functions; the per-point physics is obstacle_point.h's.
//
//   ancf_obstacle_points_kernel<S, F> (F: the list holds field obstacles; so for the footprint kernel) one wavefront per element: lanes 0..31 own the points at the current coordinates,
//                                    lanes 32..63 evaluate the same points at the start-of-step coordinates; writes
//                                    the element's rows of the contact force buffer cbuf [E][S][3], its touched flag,
//                                    the blocks C_p of a touched element and the per-obstacle shares of the element
//   ancf_obstacle_tangent_kernel<S>  one wavefront per element, leaves at once if the element is untouched: lanes own
//                                    the (i <= j) pairs and add h sum_p S_i S_j C_p to the pair's block of Kbuf
//   ancf_obstacle_gather_kernel      one thread per coefficient: ascending-element sum of its cbuf rows, g += grad Phi
//   ancf_obstacle_footprint_kernel<S> one wavefront per element: position, smallest gap and normal pressure per point
//
// No atomics: an element owns its rows of cbuf and Kbuf, a coefficient owns its row of g; every sum runs in a fixed
// order, so forces, Hessian values and resultants are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <cmath>

#include "obstacle_point.h"
#include "pair_runs.h"
#include "tlfea_internal.h"

namespace tlfea {
namespace {

constexpr int kP = kAncfObsPoints;

// coefficient vectors of element e into LDS: c[a][3] from the SoA arrays
template <int S>
__device__ __forceinline__ void stage_coefs(int E, int e, int lane, const int* __restrict__ conn,
                                            const double* __restrict__ x, const double* __restrict__ y,
                                            const double* __restrict__ z, double (*c)[3]) {
  if (lane < S) {
    const int id = conn[(size_t)lane * E + e];
    c[lane][0] = x[id];
    c[lane][1] = y[id];
    c[lane][2] = z[id];
  }
}

// r_p = sum_a S_a(p) c_a, a ascending
template <int S>
__device__ __forceinline__ void point_position(const double* __restrict__ sv, const double (*c)[3], double r[3]) {
  r[0] = r[1] = r[2] = 0.0;
#pragma unroll
  for (int a = 0; a < S; a++) {
    const double s = sv[a];
    r[0] += s * c[a][0];
    r[1] += s * c[a][1];
    r[2] += s * c[a][2];
  }
}

template <int S, bool kFields>
__global__ __launch_bounds__(64) void ancf_obstacle_points_kernel(AncfObsView v, ObstacleList L,
                                                                  const double* __restrict__ x,
                                                                  const double* __restrict__ y,
                                                                  const double* __restrict__ z,
                                                                  const double* __restrict__ xp,
                                                                  const double* __restrict__ yp,
                                                                  const double* __restrict__ zp, double h) {
  __shared__ double cur[S][3], prev[S][3], fp[kP][3];
  const int e = blockIdx.x, lane = threadIdx.x;
  const int p = lane & (kP - 1);
  const bool now = lane < kP;
  stage_coefs<S>(v.E, e, lane, v.conn, x, y, z, cur);
  stage_coefs<S>(v.E, e, lane, v.conn, xp, yp, zp, prev);
  __syncthreads();
  const double* sv = v.sval + ((size_t)v.cls[e] * kP + p) * S;
  double r[3];
  point_position<S>(sv, now ? cur : prev, r);
  // the upper half-wave hands its start-of-step position to the lane of the same point
  double q0[3];
#pragma unroll
  for (int c = 0; c < 3; c++) q0[c] = __shfl(r[c], p + kP);
  const double wk = v.w[(size_t)e * kP + p];
  double f[3] = {0.0, 0.0, 0.0}, B[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool hit = false;
  for (int j = 0; j < L.n; j++) {
    double fj[4] = {0.0, 0.0, 0.0, 0.0};
    if (now) {
      bool fric;
      const double d = obstacle_point_terms<kFields>(L.o[j], wk, r, q0, h, fj, B, fj[3], fric);
      hit = hit || d < 0.0 || fric;
      f[0] += fj[0];
      f[1] += fj[1];
      f[2] += fj[2];
    }
    // the element's share of obstacle j: a fixed butterfly over the 32 points (the upper half-wave adds zeros)
#pragma unroll
    for (int o = kP / 2; o > 0; o >>= 1)
#pragma unroll
      for (int c = 0; c < 4; c++) fj[c] += __shfl_xor(fj[c], o);
    if (lane < 4)
      v.fk[((size_t)j * v.E + e) * 4 + lane] = lane == 0 ? fj[0] : (lane == 1 ? fj[1] : (lane == 2 ? fj[2] : fj[3]));
  }
  const bool touched = __any(hit) != 0;  // wave-uniform
  if (lane == 0) v.touched[e] = touched ? 1 : 0;
  if (now) {
    fp[p][0] = f[0];
    fp[p][1] = f[1];
    fp[p][2] = f[2];
    if (touched) {
      double* b = v.blk + ((size_t)e * kP + p) * 6;
#pragma unroll
      for (int c = 0; c < 6; c++) b[c] = B[c];
    }
  }
  __syncthreads();
  // lanes own (coefficient, component) rows: sum of the 32 points in point order
  if (lane < 3 * S) {
    const int a = lane / 3, c = lane - 3 * a;
    const double* sa = v.sval + (size_t)v.cls[e] * kP * S + a;
    double acc = 0.0;
    if (touched)
      for (int q = 0; q < kP; q++) acc += sa[(size_t)q * S] * fp[q][c];
    v.cbuf[(size_t)e * 3 * S + lane] = acc;
  }
}

template <int S>
__global__ __launch_bounds__(64) void ancf_obstacle_tangent_kernel(AncfObsView v, double h, double* __restrict__ Kbuf) {
  constexpr int P = S * (S + 1) / 2;
  __shared__ double sv[kP][S], C[kP][6];
  const int e = blockIdx.x, lane = threadIdx.x;
  if (!v.touched[e]) return;  // wave-uniform: an untouched element reads and writes nothing of Kbuf
  const double* st = v.sval + (size_t)v.cls[e] * kP * S;
  for (int t = lane; t < kP * S; t += 64) (&sv[0][0])[t] = st[t];
  const double* bt = v.blk + (size_t)e * kP * 6;
  for (int t = lane; t < kP * 6; t += 64) (&C[0][0])[t] = bt[t];
  __syncthreads();
  double* Ke = Kbuf + (size_t)e * (P * 9);
  for (int pr = lane; pr < P; pr += 64) {
    int i, j;
    pair_of(S, pr, i, j);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < kP; q++) {
      const double ss = sv[q][i] * sv[q][j];
#pragma unroll
      for (int c = 0; c < 6; c++) acc[c] += ss * C[q][c];
    }
    // xx yy zz xy xz yz -> the pair's row-major 3 x 3 block (C_p is symmetric, so block (i, j) is too)
    const int ix[9] = {0, 3, 4, 3, 1, 5, 4, 5, 2};
    double* out = Ke + (size_t)pr * 9;
#pragma unroll
    for (int t = 0; t < 9; t++) out[t] += h * acc[ix[t]];
  }
}

__global__ __launch_bounds__(256) void ancf_obstacle_gather_kernel(int N, Incidence inc, const double* __restrict__ cbuf,
                                                                   double* __restrict__ fc, double* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  for (int k = inc.n2e_off[i]; k < inc.n2e_off[i + 1]; k++) {
    const double* r = cbuf + (size_t)inc.n2e[k] * 3;  // (e * S + local) * 3
    f0 += r[0];
    f1 += r[1];
    f2 += r[2];
  }
  fc[3 * (size_t)i + 0] = f0;
  fc[3 * (size_t)i + 1] = f1;
  fc[3 * (size_t)i + 2] = f2;
  if (g) {
    g[3 * (size_t)i + 0] -= f0;
    g[3 * (size_t)i + 1] -= f1;
    g[3 * (size_t)i + 2] -= f2;
  }
}

template <int S, bool kFields>
__global__ __launch_bounds__(64) void ancf_obstacle_footprint_kernel(AncfObsView v, ObstacleList L,
                                                                     const double* __restrict__ x,
                                                                     const double* __restrict__ y,
                                                                     const double* __restrict__ z,
                                                                     double* __restrict__ pts) {
  __shared__ double cur[S][3];
  const int e = blockIdx.x, lane = threadIdx.x;
  stage_coefs<S>(v.E, e, lane, v.conn, x, y, z, cur);
  __syncthreads();
  if (lane >= kP) return;
  double r[3];
  point_position<S>(v.sval + ((size_t)v.cls[e] * kP + lane) * S, cur, r);
  double gap = INFINITY, press = 0.0;
  for (int j = 0; j < L.n; j++) {
    double nrm[3];
    if (kFields && L.o[j].kind == kField) {  // takes part only where it covers the point; pressure kappa <-phi> |G|
      double phi;
      if (!field_eval(L.o[j], r, phi, nrm)) continue;
      gap = phi < gap ? phi : gap;
      if (phi < 0.0) press += L.o[j].kappa * (-phi) * sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
      continue;
    }
    const double d = obstacle_distance(L.o[j], r, nrm);
    gap = d < gap ? d : gap;
    if (d < 0.0) press += L.o[j].kappa * (-d);
  }
  double* o = pts + ((size_t)e * kP + lane) * 5;
  o[0] = r[0];
  o[1] = r[1];
  o[2] = r[2];
  o[3] = gap;
  o[4] = press;
}

}  // namespace

void launch_ancf_obstacle_points(hipStream_t s, const AncfObsView& v, const ObstacleList& L, const double* x,
                                 const double* y, const double* z, const double* xp, const double* yp, const double* zp,
                                 double h) {
  const bool f = L.has_fields();
  if (v.S == 8 && !f)
    hipLaunchKernelGGL((ancf_obstacle_points_kernel<8, false>), dim3(v.E), dim3(64), 0, s, v, L, x, y, z, xp, yp, zp, h);
  else if (v.S == 8)
    hipLaunchKernelGGL((ancf_obstacle_points_kernel<8, true>), dim3(v.E), dim3(64), 0, s, v, L, x, y, z, xp, yp, zp, h);
  else if (!f)
    hipLaunchKernelGGL((ancf_obstacle_points_kernel<16, false>), dim3(v.E), dim3(64), 0, s, v, L, x, y, z, xp, yp, zp, h);
  else
    hipLaunchKernelGGL((ancf_obstacle_points_kernel<16, true>), dim3(v.E), dim3(64), 0, s, v, L, x, y, z, xp, yp, zp, h);
}

void launch_ancf_obstacle_tangent(hipStream_t s, const AncfObsView& v, double h, double* Kbuf) {
  if (v.S == 8)
    hipLaunchKernelGGL((ancf_obstacle_tangent_kernel<8>), dim3(v.E), dim3(64), 0, s, v, h, Kbuf);
  else
    hipLaunchKernelGGL((ancf_obstacle_tangent_kernel<16>), dim3(v.E), dim3(64), 0, s, v, h, Kbuf);
}

void launch_ancf_obstacle_gather(hipStream_t s, int N, const Incidence& inc, const double* cbuf, double* fc, double* g) {
  hipLaunchKernelGGL(ancf_obstacle_gather_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, inc, cbuf, fc, g);
}

void launch_ancf_obstacle_footprint(hipStream_t s, const AncfObsView& v, const ObstacleList& L, const double* x,
                                    const double* y, const double* z, double* pts) {
  const bool f = L.has_fields();
  if (v.S == 8 && !f)
    hipLaunchKernelGGL((ancf_obstacle_footprint_kernel<8, false>), dim3(v.E), dim3(64), 0, s, v, L, x, y, z, pts);
  else if (v.S == 8)
    hipLaunchKernelGGL((ancf_obstacle_footprint_kernel<8, true>), dim3(v.E), dim3(64), 0, s, v, L, x, y, z, pts);
  else if (!f)
    hipLaunchKernelGGL((ancf_obstacle_footprint_kernel<16, false>), dim3(v.E), dim3(64), 0, s, v, L, x, y, z, pts);
  else
    hipLaunchKernelGGL((ancf_obstacle_footprint_kernel<16, true>), dim3(v.E), dim3(64), 0, s, v, L, x, y, z, pts);
}

}  // namespace tlfea
