// shape_kernels.hip -- shape sensitivities of the implicit Newton step of T10 objects: the cotangent of the
// reference coordinates of all ten nodes of every element, X_bar = - w . dg/dX.
//
//   shape_point_kernel   thread per element (sens_point_kernel's lane mapping and reads: connectivity, x, w, u, the
//                        element-fastest grad-N copy, det J) plus the material (Material by value or the per-element
//                        records).  Per point: F, D = grad w, P, dP[D] and
//                            S = (P : D + rho (N w).(N u)) I - F^T dP[D] - D^T P,
//                        then dV S G_b added into the element's ten node rows (30 accumulators).  rows [10][Epad][3],
//                        the un-compacted row form of the matrix-free pair.
//   shape_gather_kernel  matfree_gather_kernel's scheme: 8 lanes per node sum the node's rows in ascending element order
//                        (inc.n2e_off / n2e) and a fixed butterfly; X_bar [N][3] = - the sum.  A node's result depends on
//                        its own rows alone, so on no launch shape.
// No atomics: every launch is bitwise reproducible.
#include "elem_math.h"

namespace tlfea {
namespace {

constexpr bool kShapePrefetch = true;
struct RulePoints {
  double q[3][kNQ];  // the rule's points (the mass matrix's rule): x | y | z
};

// w, u [3N] interleaved; u null = no mass term.  rho of the mass term: mat.rho0 (the host passes the density the mass
// matrix was assembled with; the per-element records carry it in slot kEmRhoM).
// PREFETCH: the next point's 30 gradients are in flight while this point computes (sens_point_kernel's double buffer).
template <int MODEL, typename MT, bool PREFETCH>
__global__ __launch_bounds__(128) void shape_point_kernel(ElemView m, MT mat_in, RulePoints rp, const double* __restrict__ w,
                                                         const double* __restrict__ u, double* __restrict__ rows) {
  constexpr int S = kNN, Q = kNQ;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m.E) return;  // nothing below crosses lanes
  const Material m0 = mat_at(mat_in, e);
  const Material mat{MODEL, m0.lambda, m0.mu, m0.mu10, m0.mu01, m0.kappa, 0.0, 0.0, m0.rho0};  // the model folds at compile time
  int gn[S];
  double wn[S][3];
#pragma unroll
  for (int a = 0; a < S; a++) {
    gn[a] = m.conn[(size_t)a * m.E + e];
#pragma unroll
    for (int c = 0; c < 3; c++) wn[a][c] = w[3 * gn[a] + c];
  }
  // rho dV (N w).(N u) per point first: u is needed here only, so its 30 registers are free before the gradients arrive
  double dV[Q], mq[Q];
#pragma unroll
  for (int q = 0; q < Q; q++) {
    dV[q] = m.detJ[(size_t)e * Q + q] * m.qw[q];
    mq[q] = 0.0;
  }
  if (u != nullptr) {
    double Nq[Q][S];  // formed here as mass_values_kernel does: 50 values as kernel arguments cost 100 SGPRs (and a stack slot)
    const int edges[6][2] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {1, 3}, {2, 3}};
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const double L[4] = {1.0 - rp.q[0][q] - rp.q[1][q] - rp.q[2][q], rp.q[0][q], rp.q[1][q], rp.q[2][q]};
#pragma unroll
      for (int k = 0; k < 4; k++) Nq[q][k] = L[k] * (2.0 * L[k] - 1.0);
#pragma unroll
      for (int k = 0; k < 6; k++) Nq[q][k + 4] = 4.0 * L[edges[k][0]] * L[edges[k][1]];
    }
    double Nw[Q][3], Nu[Q][3];
#pragma unroll
    for (int q = 0; q < Q; q++)
#pragma unroll
      for (int c = 0; c < 3; c++) Nw[q][c] = Nu[q][c] = 0.0;
#pragma unroll
    for (int a = 0; a < S; a++) {
      const double ua[3] = {u[3 * gn[a]], u[3 * gn[a] + 1], u[3 * gn[a] + 2]};
#pragma unroll
      for (int q = 0; q < Q; q++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
          Nw[q][c] += Nq[q][a] * wn[a][c];
          Nu[q][c] += Nq[q][a] * ua[c];
        }
    }
#pragma unroll
    for (int q = 0; q < Q; q++) mq[q] = mat.rho0 * (Nw[q][0] * Nu[q][0] + Nw[q][1] * Nu[q][1] + Nw[q][2] * Nu[q][2]);
  }
  double xn[S][3];
#pragma unroll
  for (int a = 0; a < S; a++) {
    xn[a][0] = m.x[gn[a]];
    xn[a][1] = m.y[gn[a]];
    xn[a][2] = m.z[gn[a]];
  }
  double acc[S][3];
#pragma unroll
  for (int a = 0; a < S; a++)
#pragma unroll
    for (int c = 0; c < 3; c++) acc[a][c] = 0.0;
  double hn[S][3];
  if (PREFETCH) {
#pragma unroll
    for (int d = 0; d < 3; d++)
#pragma unroll
      for (int a = 0; a < S; a++) hn[a][d] = m.gradN_t[((size_t)d * S + a) * m.Epad + e];
  }
#pragma unroll 1
  for (int q = 0; q < Q; q++) {
    double hq[S][3];
    if (PREFETCH) {
#pragma unroll
      for (int a = 0; a < S; a++)
#pragma unroll
        for (int d = 0; d < 3; d++) hq[a][d] = hn[a][d];
      if (q + 1 < Q) {
#pragma unroll
        for (int d = 0; d < 3; d++)
#pragma unroll
          for (int a = 0; a < S; a++) hn[a][d] = m.gradN_t[((size_t)((q + 1) * 3 + d) * S + a) * m.Epad + e];
      }
    } else {
#pragma unroll
      for (int d = 0; d < 3; d++)
#pragma unroll
        for (int a = 0; a < S; a++) hq[a][d] = m.gradN_t[((size_t)(q * 3 + d) * S + a) * m.Epad + e];
    }
    double F[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, D[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int a = 0; a < S; a++)
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          F[i][j] += xn[a][i] * hq[a][j];
          D[i][j] += wn[a][i] * hq[a][j];
        }
    double P[3][3], dP[3][3];
    elastic_P(F, mat, P);
    elastic_dP(F, D, mat, dP);
    const double dv = q == 0 ? dV[0] : (q == 1 ? dV[1] : (q == 2 ? dV[2] : (q == 3 ? dV[3] : dV[4])));
    double s = q == 0 ? mq[0] : (q == 1 ? mq[1] : (q == 2 ? mq[2] : (q == 3 ? mq[3] : mq[4])));
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) s += P[i][j] * D[i][j];
    double Sm[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double t = i == j ? s : 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) t -= F[k][i] * dP[k][j] + D[k][i] * P[k][j];
        Sm[i][j] = t * dv;
      }
#pragma unroll
    for (int a = 0; a < S; a++)
#pragma unroll
      for (int i = 0; i < 3; i++) acc[a][i] += Sm[i][0] * hq[a][0] + Sm[i][1] * hq[a][1] + Sm[i][2] * hq[a][2];
  }
#pragma unroll
  for (int a = 0; a < S; a++) {
    double* r = rows + ((size_t)a * m.Epad + e) * 3;
    r[0] = acc[a][0];
    r[1] = acc[a][1];
    r[2] = acc[a][2];
  }
}

// X_bar [N][3] = -(sum of the node's rows): group g of 8 lanes of a workgroup owns node 128 blockIdx + g
__global__ __launch_bounds__(1024) void shape_gather_kernel(int N, int Epad, Incidence inc, const double* __restrict__ rows,
                                                           double* __restrict__ xbar) {
  const int l8 = threadIdx.x & 7, i = blockIdx.x * 128 + (threadIdx.x >> 3);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  if (i < N) {
    for (int k = inc.n2e_off[i] + l8; k < inc.n2e_off[i + 1]; k += 8) {
      const int code = inc.n2e[k], e = code / kNN, la = code - kNN * e;
      const double* r = rows + ((size_t)la * Epad + e) * 3;
      a0 += r[0];
      a1 += r[1];
      a2 += r[2];
    }
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) {  // every lane of the wavefront takes part: no lane has left
    a0 += __shfl_xor(a0, o);
    a1 += __shfl_xor(a1, o);
    a2 += __shfl_xor(a2, o);
  }
  if (i < N && l8 < 3) xbar[3 * (size_t)i + l8] = -((l8 == 0) ? a0 : ((l8 == 1) ? a1 : a2));
}

template <int MODEL, typename MT>
void launch_points_t(hipStream_t s, const ElemView& m, const MT& mat, const RulePoints& rp, const double* w, const double* u,
                     double* rows) {
  const dim3 grid((m.E + 127) / 128), block(128);
  hipLaunchKernelGGL((shape_point_kernel<MODEL, MT, kShapePrefetch>), grid, block, 0, s, m, mat, rp, w, u, rows);
}

}  // namespace

void launch_shape_points(hipStream_t s, const ElemView& m, const Material& mat, const double* emat, const double q[3][kNQ],
                         const double* w, const double* u, double* rows) {
  const bool mr = mat.model == kMooneyRivlin;
  RulePoints rp;
  for (int c = 0; c < 3; c++)
    for (int k = 0; k < kNQ; k++) rp.q[c][k] = q[c][k];
  if (emat) {
    const MaterialPE pe{mat, emat};
    if (mr) launch_points_t<kMooneyRivlin>(s, m, pe, rp, w, u, rows);
    else launch_points_t<kSVK>(s, m, pe, rp, w, u, rows);
  } else {
    if (mr) launch_points_t<kMooneyRivlin>(s, m, mat, rp, w, u, rows);
    else launch_points_t<kSVK>(s, m, mat, rp, w, u, rows);
  }
}

void launch_shape_gather(hipStream_t s, int N, int Epad, const Incidence& inc, const double* rows, double* xbar) {
  hipLaunchKernelGGL(shape_gather_kernel, dim3((N + 127) / 128), dim3(1024), 0, s, N, Epad, inc, rows, xbar);
}

}  // namespace tlfea
