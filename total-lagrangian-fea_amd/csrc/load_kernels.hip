// load_kernels.hip -- distributed loads (DESIGN 3h, 3h'): the consistent load of a body acceleration on any element kind,
// dead surface traction and follower pressure on the faces of ANCF-3243 beams and ANCF-3443 shells, and the follower
// pressure on the boundary faces of a T10 mesh.
//
//   body_force_kernel        one thread per coefficient row of the mass CSR: fc_i = sum_j M_ij a_j (+ the traction vector
//                            built on the host), a_j = a on position coefficients.  Runs once per change, not per step
//   ancf_pressure_kernel<S>  one wavefront per element, leaves at once if no pressure load lists the element: lanes own
//                            the Gauss points of a loaded face (current tangents, cross product, point force), then the
//                            (coefficient, component) rows of lbuf [E][S][3]
//   t10_pressure_kernel      eight lanes per LOADED boundary face (six of them active): lane q owns point q of the 6-point
//                            triangle rule (current tangents, cross product), then lane a owns node a's row of
//                            fbuf [faces][6][3].  Its gather is load_gather_kernel through the node-to-face-slot CSR
//   load_gather_kernel       one thread per coefficient: constant vector + ascending-element sum of its lbuf rows,
//                            f = the total load, g -= f
//
// No atomics: an element owns its rows of lbuf, a coefficient owns its rows of f and g; every sum runs in a fixed order,
// so the load and the gradient are bitwise reproducible.
#include <hip/hip_runtime.h>

#include "tlfea_internal.h"

namespace tlfea {
namespace {

__global__ __launch_bounds__(256) void body_force_kernel(int N, Incidence inc, const double* __restrict__ mval, int stride,
                                                         double a0, double a1, double a2, const double* __restrict__ add,
                                                         double* __restrict__ fc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  if (mval)
    for (int k = inc.off[i]; k < inc.off[i + 1]; k++) {  // ascending column order
      if (inc.cols[k] % stride) continue;               // a gradient coefficient: a_j = 0
      const double m = mval[k];
      f0 += m * a0;
      f1 += m * a1;
      f2 += m * a2;
    }
  if (add) {
    f0 += add[3 * (size_t)i + 0];
    f1 += add[3 * (size_t)i + 1];
    f2 += add[3 * (size_t)i + 2];
  }
  fc[3 * (size_t)i + 0] = f0;
  fc[3 * (size_t)i + 1] = f1;
  fc[3 * (size_t)i + 2] = f2;
}

template <int S>
__global__ __launch_bounds__(64) void ancf_pressure_kernel(AncfLoadView v, const double* __restrict__ x,
                                                           const double* __restrict__ y, const double* __restrict__ z) {
  constexpr int NF = S == 16 ? 2 : 4, P = S == 16 ? 25 : 10;
  __shared__ double cur[S][3], fq[NF][P][3];
  const int e = blockIdx.x, lane = threadIdx.x;
  const int m = v.mask[e];
  if (m == 0) return;  // wave-uniform: an element without a pressure load reads and writes nothing more
  if (lane < S) {
    const int id = v.conn[(size_t)lane * v.E + e];
    cur[lane][0] = x[id];
    cur[lane][1] = y[id];
    cur[lane][2] = z[id];
  }
  __syncthreads();
  const double* tab = v.tab + (size_t)v.cls[e] * (NF * P * 3 * S);
  for (int f = 0; f < NF; f++) {
    if (!((m >> f) & 1) || lane >= P) continue;
    // the two tangents of the face at the current coefficients, a ascending
    const double* d0 = tab + ((size_t)f * P + lane) * (3 * S) + S;
    const double* d1 = d0 + S;
    double t0[3] = {0.0, 0.0, 0.0}, t1[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < S; a++) {
      const double s0 = d0[a], s1 = d1[a];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        t0[c] += s0 * cur[a][c];
        t1[c] += s1 * cur[a][c];
      }
    }
    const double k = v.pe[(size_t)e * NF + f] * v.qw[lane];  // -(pressure) x orientation sign x quadrature weight
    fq[f][lane][0] = k * (t0[1] * t1[2] - t0[2] * t1[1]);
    fq[f][lane][1] = k * (t0[2] * t1[0] - t0[0] * t1[2]);
    fq[f][lane][2] = k * (t0[0] * t1[1] - t0[1] * t1[0]);
  }
  __syncthreads();
  // lanes own (coefficient, component) rows: sum over the points in point order, then over the faces in face order
  if (lane < 3 * S) {
    const int a = lane / 3, c = lane - 3 * a;
    double acc = 0.0;
    for (int f = 0; f < NF; f++) {
      if (!((m >> f) & 1)) continue;
      const double* sa = tab + (size_t)f * P * (3 * S) + a;
      for (int q = 0; q < P; q++) acc += sa[(size_t)q * (3 * S)] * fq[f][q][c];
    }
    v.lbuf[(size_t)e * 3 * S + lane] = acc;
  }
}

// The 6-point rule of degree 4 on the unit triangle (xi, eta, weight; the weights sum to 1/2), as t10_load_host.h.
__constant__ double kTriRule[6][3] = {
    {0.44594849091596488632, 0.44594849091596488632, 0.11169079483900573285},
    {0.10810301816807022736, 0.44594849091596488632, 0.11169079483900573285},
    {0.44594849091596488632, 0.10810301816807022736, 0.11169079483900573285},
    {0.09157621350977074346, 0.09157621350977074346, 0.05497587182766093382},
    {0.81684757298045851308, 0.09157621350977074346, 0.05497587182766093382},
    {0.09157621350977074346, 0.81684757298045851308, 0.05497587182766093382}};

// quadratic triangle: corners 0 1 2, mid-edge nodes 01 12 02
__device__ inline double tri6_shape(int a, double xi, double eta) {
  const double l0 = 1.0 - xi - eta;
  switch (a) {
    case 0: return l0 * (2 * l0 - 1);
    case 1: return xi * (2 * xi - 1);
    case 2: return eta * (2 * eta - 1);
    case 3: return 4 * l0 * xi;
    case 4: return 4 * xi * eta;
    default: return 4 * l0 * eta;
  }
}

constexpr int kT10FacesPerBlock = 8;  // 8 lanes each: one wavefront

__global__ __launch_bounds__(64) void t10_pressure_kernel(T10LoadView v, const double* __restrict__ x,
                                                          const double* __restrict__ y, const double* __restrict__ z) {
  __shared__ double cur[kT10FacesPerBlock][6][3], cq[kT10FacesPerBlock][6][3];
  const int slot = threadIdx.x >> 3, lane = threadIdx.x & 7;
  const int face = blockIdx.x * kT10FacesPerBlock + slot;
  const bool on = face < v.n_faces && lane < 6;
  if (on) {
    const int id = v.nodes[(size_t)face * 6 + lane];
    cur[slot][lane][0] = x[id];
    cur[slot][lane][1] = y[id];
    cur[slot][lane][2] = z[id];
  }
  __syncthreads();
  if (on) {  // lane = point q: the two tangents at the current positions, a ascending
    const double xi = kTriRule[lane][0], eta = kTriRule[lane][1], l0 = 1.0 - xi - eta;
    const double dx[6] = {-(4 * l0 - 1), 4 * xi - 1, 0.0, 4 * (l0 - xi), 4 * eta, -4 * eta};
    const double de[6] = {-(4 * l0 - 1), 0.0, 4 * eta - 1, -4 * xi, 4 * xi, 4 * (l0 - eta)};
    double t0[3] = {0.0, 0.0, 0.0}, t1[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        t0[c] += dx[a] * cur[slot][a][c];
        t1[c] += de[a] * cur[slot][a][c];
      }
    const double k = v.pe[face] * kTriRule[lane][2];  // -(effective pressure) x quadrature weight
    cq[slot][lane][0] = k * (t0[1] * t1[2] - t0[2] * t1[1]);
    cq[slot][lane][1] = k * (t0[2] * t1[0] - t0[0] * t1[2]);
    cq[slot][lane][2] = k * (t0[0] * t1[1] - t0[1] * t1[0]);
  }
  __syncthreads();
  if (on) {  // lane = node a: the sum over the points in point order
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
#pragma unroll
    for (int q = 0; q < 6; q++) {
      const double n = tri6_shape(lane, kTriRule[q][0], kTriRule[q][1]);
      f0 += n * cq[slot][q][0];
      f1 += n * cq[slot][q][1];
      f2 += n * cq[slot][q][2];
    }
    double* r = v.fbuf + ((size_t)face * 6 + lane) * 3;
    r[0] = f0;
    r[1] = f1;
    r[2] = f2;
  }
}

__global__ __launch_bounds__(256) void load_gather_kernel(int N, Incidence inc, const double* __restrict__ fc,
                                                          const double* __restrict__ lbuf, double* __restrict__ f,
                                                          double* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  if (fc) {
    f0 = fc[3 * (size_t)i + 0];
    f1 = fc[3 * (size_t)i + 1];
    f2 = fc[3 * (size_t)i + 2];
  }
  if (lbuf)
    for (int k = inc.n2e_off[i]; k < inc.n2e_off[i + 1]; k++) {
      const double* r = lbuf + (size_t)inc.n2e[k] * 3;  // (e * S + local) * 3
      f0 += r[0];
      f1 += r[1];
      f2 += r[2];
    }
  f[3 * (size_t)i + 0] = f0;
  f[3 * (size_t)i + 1] = f1;
  f[3 * (size_t)i + 2] = f2;
  g[3 * (size_t)i + 0] -= f0;
  g[3 * (size_t)i + 1] -= f1;
  g[3 * (size_t)i + 2] -= f2;
}

}  // namespace

void launch_body_force(hipStream_t s, int N, const Incidence& inc, const double* mval, int stride, const double a[3],
                       const double* add, double* fc) {
  hipLaunchKernelGGL(body_force_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, inc, mval, stride, a[0], a[1], a[2],
                     add, fc);
}

void launch_ancf_pressure(hipStream_t s, const AncfLoadView& v, const double* x, const double* y, const double* z) {
  if (v.S == 8)
    hipLaunchKernelGGL((ancf_pressure_kernel<8>), dim3(v.E), dim3(64), 0, s, v, x, y, z);
  else
    hipLaunchKernelGGL((ancf_pressure_kernel<16>), dim3(v.E), dim3(64), 0, s, v, x, y, z);
}

void launch_t10_pressure(hipStream_t s, const T10LoadView& v, const double* x, const double* y, const double* z) {
  if (v.n_faces <= 0) return;
  hipLaunchKernelGGL(t10_pressure_kernel, dim3((v.n_faces + kT10FacesPerBlock - 1) / kT10FacesPerBlock), dim3(64), 0, s, v,
                     x, y, z);
}

void launch_load_gather(hipStream_t s, int N, const Incidence& inc, const double* fc, const double* lbuf, double* f,
                        double* g) {
  hipLaunchKernelGGL(load_gather_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, inc, fc, lbuf, f, g);
}

}  // namespace tlfea
