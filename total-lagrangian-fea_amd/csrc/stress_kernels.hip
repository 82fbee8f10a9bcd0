// stress_kernels.hip -- stress and energy recovery of T10 objects.  Works from the positions (and an optional
// velocity) and the object's own data; touches nothing a solver reads.
//
//   stress_point_kernel   thread per element (coalesced element-fastest grad-N copy, as residual_kernel): F -> P (the
//                         residual's P: elastic_P + Kelvin-Voigt) -> Cauchy stress, strain-energy density and viscous power
//                         at the five Keast points; the element record {mean stress (6), von Mises, mean psi, mean J, V_e}
//                         and, on request, the point stresses leave through a wave-private LDS transpose (whole-line
//                         stores); the element's four volume integrals go to an element-fastest buffer for the totals
//   stress_nodal_kernel   thread per node: volume-weighted mean of the incident elements' mean stresses in ascending
//                         element order (owner computes, as fint_gather_kernel), von Mises of the averaged tensor
//   stress_partial_kernel / stress_final_kernel
//                         fixed-order two-stage sums of the element integrals and of the rows of 1/2 v.Mv
//                         (obstacle_resultant_kernel's scheme): strided per-thread sums in index order, then a fixed tree
//   ancf_stress_point_kernel
//                         the ANCF kinds (DESIGN 3f'): lanes own quadrature points.  A wavefront takes G elements of Q
//                         lanes each (shell <16,48>: 1 x 48, beam <8,12>: 5 x 12); the elements' coefficient vectors sit in
//                         the wavefront's LDS slice, every lane streams its own contiguous 3 x S gradient run into F (and
//                         Fdot) and forms P, sigma, psi and P_vis:Fdot of its point; the element sums are a fixed halving
//                         tree over the element's lanes (Q = 3 * 2^k: Q/2, Q/4, ..., 3, then lanes 0 + 1 + 2)
//   stress_node_gather_kernel
//                         thread per mesh node over a node -> element list (ascending elements): the ANCF nodal stress
// No atomics: every launch is bitwise reproducible.
#include <type_traits>

#include "elem_math.h"

namespace tlfea {
namespace {

constexpr int kPtRow = 31;   // LDS doubles per lane behind the 30 point-stress doubles of an element (odd: no bank pile-up)
constexpr int kElRow = 11;   // ... behind its 10-double record
constexpr int kRed = 256;    // threads of a reduction block

// stored order: xx yy zz xy yz zx
__device__ __forceinline__ double von_mises6(const double s[6]) {
  const double a = s[0] - s[1], b = s[1] - s[2], c = s[2] - s[0];
  return sqrt(0.5 * (a * a + b * b + c * c) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]));
}

// Strain-energy density per reference volume whose derivative is elastic_P: St.Venant-Kirchhoff
// 1/2 lambda (tr E)^2 + mu E:E; compressible Mooney-Rivlin mu10 (J^-2/3 I1 - 3) + mu01 (J^-4/3 I2 - 3) + 1/2 kappa (J - 1)^2
// with I1, I2 as in mr_state.
__device__ __forceinline__ double elastic_psi(const double F[3][3], const Material& mat) {
  double C[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[i][j] = F[0][i] * F[0][j] + F[1][i] * F[1][j] + F[2][i] * F[2][j];
  if (mat.model == kMooneyRivlin) {
    const double I1 = C[0][0] + C[1][1] + C[2][2];
    double trC2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) trC2 += C[i][k] * C[k][i];
    const double I2 = 0.5 * (I1 * I1 - trC2);
    const double J = det3(F);
    const double J13 = cbrt(J);
    const double Jm23 = 1.0 / (J13 * J13);
    return mat.mu10 * (Jm23 * I1 - 3.0) + mat.mu01 * (Jm23 * Jm23 * I2 - 3.0) + 0.5 * mat.kappa * (J - 1.0) * (J - 1.0);
  }
  double trE = 0.0, EE = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double Eij = 0.5 * (C[i][j] - (i == j ? 1.0 : 0.0));
      if (i == j) trE += Eij;
      EE += Eij * Eij;
    }
  return 0.5 * mat.lambda * trE * trE + mat.mu * EE;
}

// pts [E][5][6], erec [E][10], contrib [4][Epad] = sum_q {psi, P_vis:Fdot, 1, J} dV.  MT as residual_kernel.
template <bool POINTS, class MT>
__global__ __launch_bounds__(128) void stress_point_kernel(ElemView m, MT mat_in, const double* __restrict__ v,
                                                          double* __restrict__ pts, double* __restrict__ erec,
                                                          double* __restrict__ contrib) {
  constexpr int S = kNN, Q = kNQ;
  constexpr int kSlice = 64 * (POINTS ? kPtRow : kElRow);
  __shared__ double tr_all[2 * kSlice];
  double* tr = tr_all + (threadIdx.x >> 6) * kSlice;  // this wavefront's slice
  const int lane = threadIdx.x & 63;
  const int e0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63);  // first element of this wavefront
  const int e_raw = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = e_raw < m.E ? e_raw : m.E - 1;  // lanes past the end stay for the transposes; their stores are masked
  const Material mat = mat_at(mat_in, e);
  const bool damp = (v != nullptr) && (mat.eta != 0.0 || mat.lamd != 0.0);  // residual_kernel's condition
  int gn[S];
  double xn[S][3];
#pragma unroll
  for (int a = 0; a < S; a++) {
    gn[a] = m.conn[(size_t)a * m.E + e];
    xn[a][0] = m.x[gn[a]];
    xn[a][1] = m.y[gn[a]];
    xn[a][2] = m.z[gn[a]];
  }
  double sb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, W = 0.0, D = 0.0, V = 0.0, Vc = 0.0;
  // as residual_kernel: the registers of x and of two points' gradients leave one wavefront per SIMD, so the next
  // point's gradients are in flight while this point computes
  double hn[S][3];
#pragma unroll
  for (int d = 0; d < 3; d++)
#pragma unroll
    for (int a = 0; a < S; a++) hn[a][d] = m.gradN_t[((size_t)d * S + a) * m.Epad + e];
#pragma unroll 1
  for (int q = 0; q < Q; q++) {
    double hq[S][3];
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
    double F[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int a = 0; a < S; a++)
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) F[i][j] += xn[a][i] * hq[a][j];
    double P[3][3];
    elastic_P(F, mat, P);
    double pvis = 0.0;
    if (damp) {
      // Fdot = sum v_a (x) h_a ; Edot = sym(Fdot^T F) ; S = 2 eta Edot + lamd tr(Edot) I ; P_vis = F S (residual_kernel)
      double Fd[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
      for (int a = 0; a < S; a++) {
        const double va[3] = {v[3 * gn[a] + 0], v[3 * gn[a] + 1], v[3 * gn[a] + 2]};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) Fd[i][j] += va[i] * hq[a][j];
      }
      double Ed[3][3];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          double a1 = 0.0, a2 = 0.0;
#pragma unroll
          for (int k = 0; k < 3; k++) {
            a1 += Fd[k][i] * F[k][j];
            a2 += F[k][i] * Fd[k][j];
          }
          Ed[i][j] = 0.5 * (a1 + a2);
        }
      const double trEd = Ed[0][0] + Ed[1][1] + Ed[2][2];
      double Sv[3][3];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Sv[i][j] = 2.0 * mat.eta * Ed[i][j] + (i == j ? mat.lamd * trEd : 0.0);
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 3; k++) s += F[i][k] * Sv[k][j];
          P[i][j] += s;
          pvis += s * Fd[i][j];
        }
    }
    const double J = det3(F);
    const double iJ = 1.0 / J;
    // sigma = P F^T / J, stored xx yy zz xy yz zx
    const int si[6] = {0, 1, 2, 0, 1, 2}, sj[6] = {0, 1, 2, 1, 2, 0};
    double sig[6];
#pragma unroll
    for (int c = 0; c < 6; c++)
      sig[c] = (P[si[c]][0] * F[sj[c]][0] + P[si[c]][1] * F[sj[c]][1] + P[si[c]][2] * F[sj[c]][2]) * iJ;
    const double psi = elastic_psi(F, mat);
    const double dV = m.detJ[(size_t)e * Q + q] * m.qw[q];
#pragma unroll
    for (int c = 0; c < 6; c++) sb[c] += sig[c] * dV;
    W += psi * dV;
    D += pvis * dV;
    V += dV;
    Vc += J * dV;
    if (POINTS) {
#pragma unroll
      for (int c = 0; c < 6; c++) tr[lane * kPtRow + q * 6 + c] = sig[c];
    }
  }
  if (POINTS) {
    // the wavefront's 64 x 30 point-stress doubles are 15 360 contiguous bytes: 512-byte store instructions
    wave_sync();
    double* out = pts + (size_t)e0 * 30;
#pragma unroll 6
    for (int j = 0; j < 30; j++) {
      const int idx = lane + 64 * j, el = idx / 30, c = idx - 30 * el;
      const double val = tr[el * kPtRow + c];
      if (e0 + el < m.E) out[idx] = val;
    }
    wave_sync();
  }
  const double iV = 1.0 / V;
  double rec[10];
#pragma unroll
  for (int c = 0; c < 6; c++) rec[c] = sb[c] * iV;
  rec[6] = von_mises6(rec);
  rec[7] = W * iV;
  rec[8] = Vc * iV;
  rec[9] = V;
#pragma unroll
  for (int c = 0; c < 10; c++) tr[lane * kElRow + c] = rec[c];
  wave_sync();
  double* out = erec + (size_t)e0 * 10;
#pragma unroll
  for (int j = 0; j < 10; j++) {
    const int idx = lane + 64 * j, el = idx / 10, c = idx - 10 * el;
    const double val = tr[el * kElRow + c];
    if (e0 + el < m.E) out[idx] = val;
  }
  if (e_raw < m.E) {
    contrib[(size_t)0 * m.Epad + e] = W;
    contrib[(size_t)1 * m.Epad + e] = D;
    contrib[(size_t)2 * m.Epad + e] = V;
    contrib[(size_t)3 * m.Epad + e] = Vc;
  }
}

// ---- ANCF beams and shells: lanes own quadrature points ---------------------------------------------------------------------
constexpr int kAncfPtRow = 7;  // LDS doubles per lane behind its 6 point-stress doubles (odd: no bank pile-up)

// pts [E][Q][6], erec [E][10], contrib [4][Epad] as stress_point_kernel.  gradN [E][Q][3][S]: lane (g, q) reads the run of (e0 + g, q).
template <int S, int Q, bool POINTS>
__global__ __launch_bounds__(64 * kAncfWaves) void ancf_stress_point_kernel(ElemView m, Material mat,
                                                                           const double* __restrict__ v,
                                                                           double* __restrict__ pts,
                                                                           double* __restrict__ erec,
                                                                           double* __restrict__ contrib) {
  constexpr int G = 64 / Q;            // elements of a wavefront
  constexpr int kRow = 3 * S + 1;      // LDS doubles of an element's coefficient vectors (+1: the G rows start on different banks)
  __shared__ double xs_all[kAncfWaves][G * kRow], vs_all[kAncfWaves][G * kRow];
  __shared__ double tr_all[kAncfWaves][POINTS ? 64 * kAncfPtRow : G * 10];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e0 = (blockIdx.x * kAncfWaves + w) * G;  // first element of this wavefront
  if (e0 >= m.E) return;                             // the whole wavefront: nothing below synchronises across wavefronts
  double *xs = xs_all[w], *vs = vs_all[w], *tr = tr_all[w];
  const int n_el = min(G, m.E - e0);                 // elements of this wavefront
  const bool damp = (v != nullptr) && (mat.eta != 0.0 || mat.lamd != 0.0);  // residual_kernel's condition
  // the elements' coefficient vectors (and velocities), once per element
  for (int idx = lane; idx < n_el * S; idx += 64) {
    const int el = idx / S, a = idx - el * S;
    const int c = m.conn[(size_t)a * m.E + e0 + el];
    double* xo = xs + el * kRow + 3 * a;
    xo[0] = m.x[c];
    xo[1] = m.y[c];
    xo[2] = m.z[c];
    if (damp) {
      double* vo = vs + el * kRow + 3 * a;
      vo[0] = v[3 * c];
      vo[1] = v[3 * c + 1];
      vo[2] = v[3 * c + 2];
    }
  }
  wave_sync();
  const int g_raw = lane / Q, p = lane - g_raw * Q;
  const bool active = g_raw < n_el;       // lanes past the wavefront's elements recompute element e0 and contribute zeros
  const int g = active ? g_raw : 0, e = e0 + g;
  const double2* gr = reinterpret_cast<const double2*>(m.gradN + ((size_t)e * Q + p) * (3 * S));  // 3 S doubles: 16-byte aligned
  const double* xe = xs + g * kRow;
  const double* ve = vs + g * kRow;
  double F[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Fd[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
  for (int d = 0; d < 3; d++)
#pragma unroll
    for (int a = 0; a < S; a += 2) {
      const double2 h = gr[(d * S + a) >> 1];
#pragma unroll
      for (int i = 0; i < 3; i++) F[i][d] += xe[3 * a + i] * h.x + xe[3 * a + 3 + i] * h.y;
      if (damp) {
#pragma unroll
        for (int i = 0; i < 3; i++) Fd[i][d] += ve[3 * a + i] * h.x + ve[3 * a + 3 + i] * h.y;
      }
    }
  double P[3][3];
  elastic_P(F, mat, P);
  double pvis = 0.0;
  if (damp) {
    // Edot = sym(Fdot^T F) ; S = 2 eta Edot + lamd tr(Edot) I ; P_vis = F S (residual_kernel)
    double Ed[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          a1 += Fd[k][i] * F[k][j];
          a2 += F[k][i] * Fd[k][j];
        }
        Ed[i][j] = 0.5 * (a1 + a2);
      }
    const double trEd = Ed[0][0] + Ed[1][1] + Ed[2][2];
    double Sv[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Sv[i][j] = 2.0 * mat.eta * Ed[i][j] + (i == j ? mat.lamd * trEd : 0.0);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += F[i][k] * Sv[k][j];
        P[i][j] += s;
        pvis += s * Fd[i][j];
      }
  }
  const double J = det3(F);
  const double iJ = 1.0 / J;
  const int si[6] = {0, 1, 2, 0, 1, 2}, sj[6] = {0, 1, 2, 1, 2, 0};  // sigma = P F^T / J, stored xx yy zz xy yz zx
  double sig[6];
#pragma unroll
  for (int c = 0; c < 6; c++)
    sig[c] = (P[si[c]][0] * F[sj[c]][0] + P[si[c]][1] * F[sj[c]][1] + P[si[c]][2] * F[sj[c]][2]) * iJ;
  const double psi = elastic_psi(F, mat);
  const double dV = active ? m.detJ[(size_t)e * Q + p] * m.qw[p] : 0.0;
  if (POINTS) {
    // the wavefront's n_el x Q x 6 point-stress doubles are contiguous (lane = g Q + q): whole-line stores
#pragma unroll
    for (int c = 0; c < 6; c++) tr[lane * kAncfPtRow + c] = sig[c];
    wave_sync();
    double* out = pts + (size_t)e0 * Q * 6;
    const int n_out = n_el * Q * 6;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const int idx = lane + 64 * j, l = idx / 6, c = idx - 6 * l;
      if (idx < n_out) out[idx] = tr[l * kAncfPtRow + c];
    }
    wave_sync();
  }
  double rec[10];
#pragma unroll
  for (int c = 0; c < 6; c++) rec[c] = elem_lane_sum<Q>(sig[c] * dV, lane, p);
  const double W = elem_lane_sum<Q>(psi * dV, lane, p);
  const double D = elem_lane_sum<Q>(pvis * dV, lane, p);
  const double V = elem_lane_sum<Q>(dV, lane, p);
  const double Vc = elem_lane_sum<Q>(J * dV, lane, p);
  if (active && p == 0) {
    const double iV = 1.0 / V;
#pragma unroll
    for (int c = 0; c < 6; c++) rec[c] *= iV;
    rec[6] = von_mises6(rec);
    rec[7] = W * iV;
    rec[8] = Vc * iV;
    rec[9] = V;
#pragma unroll
    for (int c = 0; c < 10; c++) tr[g * 10 + c] = rec[c];
    contrib[(size_t)0 * m.Epad + e] = W;
    contrib[(size_t)1 * m.Epad + e] = D;
    contrib[(size_t)2 * m.Epad + e] = V;
    contrib[(size_t)3 * m.Epad + e] = Vc;
  }
  wave_sync();
  if (lane < n_el * 10) erec[(size_t)e0 * 10 + lane] = tr[lane];  // the wavefront's records are contiguous
}

// nodal [n_nodes][7] of the ANCF kinds: node -> element list (off [n_nodes + 1], el ascending per node) instead of the
// coefficient-level Incidence; otherwise stress_nodal_kernel
__global__ __launch_bounds__(kRed) void stress_node_gather_kernel(int n_nodes, const int* __restrict__ off,
                                                                 const int* __restrict__ el,
                                                                 const double* __restrict__ erec,
                                                                 double* __restrict__ nodal) {
  __shared__ double st[kRed * 7];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * kRed, i = i0 + t;
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w = 0.0;
  if (i < n_nodes) {
    for (int k = off[i]; k < off[i + 1]; k++) {
      const double* r = erec + (size_t)el[k] * 10;
      const double Ve = r[9];
#pragma unroll
      for (int c = 0; c < 6; c++) a[c] += Ve * r[c];
      w += Ve;
    }
    if (w > 0.0) {  // a node of no element keeps zeros
      const double iw = 1.0 / w;
#pragma unroll
      for (int c = 0; c < 6; c++) a[c] *= iw;
    }
    a[6] = von_mises6(a);
  }
#pragma unroll
  for (int c = 0; c < 7; c++) st[t * 7 + c] = a[c];
  __syncthreads();
  const int n_here = min(kRed, n_nodes - i0) * 7;
  for (int k = t; k < n_here; k += kRed) nodal[(size_t)i0 * 7 + k] = st[k];
}

// nodal [N][7] = sigma_i (6) | von Mises of sigma_i; a block's 256 x 7 doubles are contiguous and leave through LDS
__global__ __launch_bounds__(kRed) void stress_nodal_kernel(int N, Incidence inc, const double* __restrict__ erec,
                                                           double* __restrict__ nodal) {
  __shared__ double st[kRed * 7];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * kRed, i = i0 + t;
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w = 0.0;
  if (i < N) {
    for (int k = inc.n2e_off[i]; k < inc.n2e_off[i + 1]; k++) {
      const double* r = erec + (size_t)(inc.n2e[k] / kNN) * 10;
      const double Ve = r[9];
#pragma unroll
      for (int c = 0; c < 6; c++) a[c] += Ve * r[c];
      w += Ve;
    }
    if (w > 0.0) {  // a node of no element keeps zeros
      const double iw = 1.0 / w;
#pragma unroll
      for (int c = 0; c < 6; c++) a[c] *= iw;
    }
    a[6] = von_mises6(a);
  }
#pragma unroll
  for (int c = 0; c < 7; c++) st[t * 7 + c] = a[c];
  __syncthreads();
  const int n_here = min(kRed, N - i0) * 7;
  for (int k = t; k < n_here; k += kRed) nodal[(size_t)i0 * 7 + k] = st[k];
}

// Blocks [0, nbE) sum the element integrals of `perE` consecutive elements each, blocks [nbE, nbE + nbN) the rows
// 1/2 v_i . (M v)_i of `perN` consecutive nodes; partial[b][5] = {strain energy, kinetic energy, viscous power,
// reference volume, current volume} (zeros in the columns a block does not own).
__global__ __launch_bounds__(kRed) void stress_partial_kernel(int E, int Epad, const double* __restrict__ contrib, int nbE,
                                                             int perE, int N, Incidence inc,
                                                             const double* __restrict__ mval,
                                                             const double* __restrict__ v, int perN,
                                                             double* __restrict__ partial) {
  __shared__ double acc[5][kRed];
  const int b = blockIdx.x, t = threadIdx.x;
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (b < nbE) {
    const int end = min(E, (b + 1) * perE);
    for (int e = b * perE + t; e < end; e += kRed) {
      a[0] += contrib[(size_t)0 * Epad + e];
      a[2] += contrib[(size_t)1 * Epad + e];
      a[3] += contrib[(size_t)2 * Epad + e];
      a[4] += contrib[(size_t)3 * Epad + e];
    }
  } else {
    const int r0 = (b - nbE) * perN, end = min(N, r0 + perN);
    for (int i = r0 + t; i < end; i += kRed) {
      const double vi[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
      double s = 0.0;
      for (int k = inc.off[i]; k < inc.off[i + 1]; k++) {
        const int c = inc.cols[k];
        s += mval[k] * (vi[0] * v[3 * c] + vi[1] * v[3 * c + 1] + vi[2] * v[3 * c + 2]);
      }
      a[1] += 0.5 * s;
    }
  }
  for (int c = 0; c < 5; c++) acc[c][t] = a[c];
  __syncthreads();
  for (int s = kRed / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int c = 0; c < 5; c++) acc[c][t] += acc[c][t + s];
    __syncthreads();
  }
  if (t < 5) partial[(size_t)b * 5 + t] = acc[t][0];
}

__global__ __launch_bounds__(kRed) void stress_final_kernel(int nb, const double* __restrict__ partial,
                                                           double* __restrict__ out) {
  __shared__ double acc[5][kRed];
  const int t = threadIdx.x;
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = t; b < nb; b += kRed)
    for (int c = 0; c < 5; c++) a[c] += partial[(size_t)b * 5 + c];
  for (int c = 0; c < 5; c++) acc[c][t] = a[c];
  __syncthreads();
  for (int s = kRed / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int c = 0; c < 5; c++) acc[c][t] += acc[c][t + s];
    __syncthreads();
  }
  if (t < 5) out[t] = acc[t][0];
}

// blocks of a partial-sum stage over n items: at most kStressMaxPart / 2, each a whole number of 256-item strides
inline void part_split(int n, int* nb, int* per) {
  const int strides = (n + kRed - 1) / kRed;
  int b = strides < kStressMaxPart / 2 ? strides : kStressMaxPart / 2;
  if (b < 1) b = 1;
  *per = ((strides + b - 1) / b) * kRed;
  if (*per < kRed) *per = kRed;
  b = (n + *per - 1) / *per;
  *nb = b < 1 ? 1 : b;
}

template <class MT>
void launch_points_t(hipStream_t s, const ElemView& m, const MT& mat, const double* v, double* pts, double* erec,
                     double* contrib) {
  const dim3 grid((m.E + 127) / 128), block(128);
  if (pts) hipLaunchKernelGGL((stress_point_kernel<true, MT>), grid, block, 0, s, m, mat, v, pts, erec, contrib);
  else hipLaunchKernelGGL((stress_point_kernel<false, MT>), grid, block, 0, s, m, mat, v, pts, erec, contrib);
}

}  // namespace

void launch_stress_points(hipStream_t s, const ElemView& m, const Material& mat, const double* emat, const double* v,
                          double* pts, double* erec, double* contrib) {
  if (emat) launch_points_t(s, m, MaterialPE{mat, emat}, v, pts, erec, contrib);
  else launch_points_t(s, m, mat, v, pts, erec, contrib);
}

template <int S, int Q>
static void launch_ancf_points_t(hipStream_t s, const ElemView& m, const Material& mat, const double* v, double* pts,
                                 double* erec, double* contrib) {
  const int per_block = kAncfWaves * (64 / Q);
  const dim3 grid((m.E + per_block - 1) / per_block), block(64 * kAncfWaves);
  if (pts) hipLaunchKernelGGL((ancf_stress_point_kernel<S, Q, true>), grid, block, 0, s, m, mat, v, pts, erec, contrib);
  else hipLaunchKernelGGL((ancf_stress_point_kernel<S, Q, false>), grid, block, 0, s, m, mat, v, pts, erec, contrib);
}

void launch_ancf_stress_points(hipStream_t s, const ElemView& m, const Material& mat, const double* v, double* pts,
                               double* erec, double* contrib) {
  if (m.S == 8) launch_ancf_points_t<8, 12>(s, m, mat, v, pts, erec, contrib);
  else launch_ancf_points_t<16, 48>(s, m, mat, v, pts, erec, contrib);
}

void launch_stress_node_gather(hipStream_t s, int n_nodes, const int* off, const int* el, const double* erec,
                               double* nodal) {
  hipLaunchKernelGGL(stress_node_gather_kernel, dim3((n_nodes + kRed - 1) / kRed), dim3(kRed), 0, s, n_nodes, off, el, erec,
                     nodal);
}

void launch_stress_nodal(hipStream_t s, int N, const Incidence& inc, const double* erec, double* nodal) {
  hipLaunchKernelGGL(stress_nodal_kernel, dim3((N + kRed - 1) / kRed), dim3(kRed), 0, s, N, inc, erec, nodal);
}

void launch_stress_totals(hipStream_t s, int E, int Epad, const double* contrib, int N, const Incidence& inc,
                          const double* mval, const double* v, double* partial, double* out5) {
  int nbE, perE, nbN = 0, perN = kRed;
  part_split(E, &nbE, &perE);
  if (v) part_split(N, &nbN, &perN);
  hipLaunchKernelGGL(stress_partial_kernel, dim3(nbE + nbN), dim3(kRed), 0, s, E, Epad, contrib, nbE, perE, N, inc, mval,
                     v, perN, partial);
  hipLaunchKernelGGL(stress_final_kernel, dim3(1), dim3(kRed), 0, s, nbE + nbN, partial, out5);
}

}  // namespace tlfea
