// stress_recovery_kernels.hip -- recovered nodal stress, principal stresses and the ZZ error indicator of T10 objects
// (DESIGN 3f'').  Works from the stored point stresses [E][5][6] of a stress recovery (or caller-given ones) and the object's
// own data; touches nothing a solver reads.
//
//   recovery_elem_kernel    thread per element.  The wavefront's 64 x 30 point doubles arrive through a wave-private LDS
//                           transpose (whole-line loads); the element record [32] = the four V_e-weighted vertex
//                           extrapolations (24) | V_e | 0 | the volume-weighted mean stress (6) leaves the same way
//   recovery_nodal_kernel   thread per node over the incidence list in ascending element order (owner computes, as
//                           stress_nodal_kernel): 48 bytes of the element record per vertex incidence, 2 x 48 per
//                           mid-edge incidence (the mean of its two vertices' rows), V_e beside them
//   recovery_nodal_direct_kernel
//                           the same sum straight from the 240-byte point block of every incidence (the form measured
//                           against the one above, DESIGN 3f''; the timing entry point runs it, the recovery does not)
//   principal_kernel        thread per tensor: cyclic Jacobi in fp64, a fixed number of sweeps
//   zz_error_kernel         thread per element: e_q = sum_a N_a(xi_q) sigma*_a - sigma_q at the rule's points,
//                           eta_e^2, n_e^2 and the clamp flag plane-major [3][Epad]
// The totals are launch_adj_sums' fixed-order two-stage sums.  No atomics: every launch is bitwise reproducible.
#include "elem_math.h"

namespace tlfea {
namespace {

constexpr int kPtRow = 31;   // LDS doubles per lane behind the 30 point-stress doubles of an element (odd: no bank pile-up)
constexpr int kRecRow = 33;  // ... behind its kRecoveryRec-double record
constexpr int kNod = 256;    // threads of a nodal block
constexpr int kJacobiSweeps = 8;
static_assert(kRecoveryRec == 32, "record layout: 24 vertex values, V_e, a zero, 6 mean values");

// stored order: xx yy zz xy yz zx
__device__ __forceinline__ double von_mises6(const double s[6]) {
  const double a = s[0] - s[1], b = s[1] - s[2], c = s[2] - s[0];
  return sqrt(0.5 * (a * a + b * b + c * c) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]));
}

// the 64 x 30 point doubles of the elements e0 .. e0 + 63 into tr (row stride kPtRow); rows past E stay unwritten
__device__ __forceinline__ void load_point_rows(const double* __restrict__ pts, int e0, int E, int lane, double* tr) {
  const double* in = pts + (size_t)e0 * 30;
#pragma unroll 6
  for (int j = 0; j < 30; j++) {
    const int idx = lane + 64 * j, el = idx / 30, c = idx - 30 * el;
    if (e0 + el < E) tr[el * kPtRow + c] = in[idx];
  }
}

__global__ __launch_bounds__(128) void recovery_elem_kernel(int E, const double* __restrict__ detJ, RecoveryTable tb,
                                                           const double* __restrict__ pts, double* __restrict__ rec) {
  __shared__ double tr_all[2 * 64 * kRecRow];
  double* tr = tr_all + (threadIdx.x >> 6) * (64 * kRecRow);  // this wavefront's slice
  const int lane = threadIdx.x & 63;
  const int e0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63);  // first element of this wavefront
  if (e0 >= E) return;                                           // the whole wavefront: nothing below crosses wavefronts
  const int e = min(e0 + lane, E - 1);  // lanes past the end stay for the transposes; their stores are masked
  load_point_rows(pts, e0, E, lane, tr);
  wave_sync();
  double sig[kNQ][6], dV[kNQ], V = 0.0;
  const double* row = tr + (e - e0) * kPtRow;
#pragma unroll
  for (int q = 0; q < kNQ; q++) {
#pragma unroll
    for (int c = 0; c < 6; c++) sig[q][c] = row[q * 6 + c];
    dV[q] = detJ[(size_t)e * kNQ + q] * tb.qw[q];
    V += dV[q];
  }
  double out[kRecoveryRec];
#pragma unroll
  for (int b = 0; b < 4; b++)
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < kNQ; q++) s += tb.T[b][q] * sig[q][c];
      out[b * 6 + c] = V * s;
    }
  out[24] = V;
  out[25] = 0.0;
  const double iV = 1.0 / V;
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kNQ; q++) s += sig[q][c] * dV[q];
    out[26 + c] = s * iV;
  }
  wave_sync();  // every lane has read its point row: the slice is free for the records
#pragma unroll
  for (int c = 0; c < kRecoveryRec; c++) tr[lane * kRecRow + c] = out[c];
  wave_sync();
  double* dst = rec + (size_t)e0 * kRecoveryRec;
#pragma unroll 8
  for (int j = 0; j < kRecoveryRec; j++) {
    const int idx = lane + 64 * j, el = idx / kRecoveryRec, c = idx - kRecoveryRec * el;
    if (e0 + el < E) dst[idx] = tr[el * kRecRow + c];
  }
}

// a block's 256 x 7 doubles {sigma*_i (6) | its von Mises} are contiguous and leave through LDS
__device__ __forceinline__ void store_nodal_rows(double a[7], double w, bool live, int N, int i0, int t, double* st,
                                                 double* __restrict__ nodal) {
  if (live) {
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
  const int n_here = min(kNod, N - i0) * 7;
  for (int k = t; k < n_here; k += kNod) nodal[(size_t)i0 * 7 + k] = st[k];
}

__global__ __launch_bounds__(kNod) void recovery_nodal_kernel(int N, Incidence inc, const double* __restrict__ rec,
                                                             double* __restrict__ nodal) {
  __shared__ double st[kNod * 7];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * kNod, i = i0 + t;
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w = 0.0;
  if (i < N) {
    for (int k = inc.n2e_off[i]; k < inc.n2e_off[i + 1]; k++) {
      const int code = inc.n2e[k], e = code / kNN, la = code - kNN * e;
      const double* r = rec + (size_t)e * kRecoveryRec;
      // One path for every lane: a vertex takes its own row twice (0.5 (u + u) = u exactly), a mid-edge node the rows of
      // its two vertices; local mid-edge order (0,1) (1,2) (0,2) (0,3) (1,3) (2,3), two bits per entry.  Rows are 48 b bytes
      // into a 256-byte record.
      const int j = la < 4 ? 0 : 2 * (la - 4), b0 = la < 4 ? la : (0x904 >> j) & 3, b1 = la < 4 ? la : (0xFE9 >> j) & 3;
      const double2* p = reinterpret_cast<const double2*>(r + 6 * b0);
      const double2* q = reinterpret_cast<const double2*>(r + 6 * b1);
      const double2 u0 = p[0], u1 = p[1], u2 = p[2], v0 = q[0], v1 = q[1], v2 = q[2];
      const double Ve = r[24];
      a[0] += 0.5 * (u0.x + v0.x); a[1] += 0.5 * (u0.y + v0.y); a[2] += 0.5 * (u1.x + v1.x);
      a[3] += 0.5 * (u1.y + v1.y); a[4] += 0.5 * (u2.x + v2.x); a[5] += 0.5 * (u2.y + v2.y);
      w += Ve;
    }
  }
  store_nodal_rows(a, w, i < N, N, i0, t, st, nodal);
}

__global__ __launch_bounds__(kNod) void recovery_nodal_direct_kernel(int N, Incidence inc, RecoveryTable tb,
                                                                    const double* __restrict__ pts,
                                                                    const double* __restrict__ rec,
                                                                    double* __restrict__ nodal) {
  __shared__ double st[kNod * 7];
  __shared__ double Ts[kNN * kNQ];
  const int t = threadIdx.x;
  if (t < kNN * kNQ) Ts[t] = tb.T[t / kNQ][t % kNQ];
  __syncthreads();
  const int i0 = blockIdx.x * kNod, i = i0 + t;
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w = 0.0;
  if (i < N) {
    for (int k = inc.n2e_off[i]; k < inc.n2e_off[i + 1]; k++) {
      const int code = inc.n2e[k], e = code / kNN, la = code - kNN * e;
      const double2* p = reinterpret_cast<const double2*>(pts + (size_t)e * 30);  // 240-byte blocks: 16-byte aligned
      const double Ve = rec[(size_t)e * kRecoveryRec + 24];
      double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < kNQ; q++) {
        const double tq = Ts[la * kNQ + q];
        const double2 u0 = p[3 * q], u1 = p[3 * q + 1], u2 = p[3 * q + 2];
        s[0] += tq * u0.x; s[1] += tq * u0.y; s[2] += tq * u1.x; s[3] += tq * u1.y; s[4] += tq * u2.x; s[5] += tq * u2.y;
      }
#pragma unroll
      for (int c = 0; c < 6; c++) a[c] += Ve * s[c];
      w += Ve;
    }
  }
  store_nodal_rows(a, w, i < N, N, i0, t, st, nodal);
}

// one Jacobi rotation that annihilates A[P][Q] (P < Q); R = the third index.  V's columns are the vectors.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double A[3][3], double V[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  // tan of the smaller rotation angle; past |theta| = 1e150 theta^2 leaves the range and 1 / (2 theta) is exact to an ulp
  const double at = fabs(theta);
  const double tmag = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
  const double tn = theta < 0.0 ? -tmag : tmag;
  const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
  A[P][P] -= tn * apq;
  A[Q][Q] += tn * apq;
  A[P][Q] = A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
}

__device__ __forceinline__ void swap_pair(double& a, double& b) { const double t = a; a = b; b = t; }

// tensor k = src[k * stride + offset .. + 6] (xx yy zz xy yz zx) -> val [n][4] = s1 >= s2 >= s3 | (s1 - s3) / 2 and, unless
// null, dir [n][9] = the unit vectors of s1, s2, s3 as rows of a right-handed frame
__global__ __launch_bounds__(256) void principal_kernel(int n, const double* __restrict__ src, int stride, int offset,
                                                       double* __restrict__ val, double* __restrict__ dir) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double* s = src + (size_t)k * stride + offset;
  double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  A[0][0] = s[0]; A[1][1] = s[1]; A[2][2] = s[2];
  A[0][1] = A[1][0] = s[3];
  A[1][2] = A[2][1] = s[4];
  A[0][2] = A[2][0] = s[5];
#pragma unroll 1
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
    jacobi_rotate<0, 1>(A, V);
    jacobi_rotate<0, 2>(A, V);
    jacobi_rotate<1, 2>(A, V);
  }
  double ev[3] = {A[0][0], A[1][1], A[2][2]};
  // descending order: a fixed three-exchange network that carries the columns of V along
#define TLFEA_ORDER(I, J)                                      \
  if (ev[I] < ev[J]) {                                         \
    swap_pair(ev[I], ev[J]);                                   \
    for (int r = 0; r < 3; r++) swap_pair(V[r][I], V[r][J]);   \
  }
  TLFEA_ORDER(0, 1)
  TLFEA_ORDER(1, 2)
  TLFEA_ORDER(0, 1)
#undef TLFEA_ORDER
  double2* vo = reinterpret_cast<double2*>(val + (size_t)k * 4);
  vo[0] = make_double2(ev[0], ev[1]);
  vo[1] = make_double2(ev[2], 0.5 * (ev[0] - ev[2]));
  if (dir) {
    // rotations keep det V = +1 and an exchange of two columns flips it: the third vector takes the sign of n1 x n2
    const double cx = V[1][0] * V[2][1] - V[2][0] * V[1][1], cy = V[2][0] * V[0][1] - V[0][0] * V[2][1],
                 cz = V[0][0] * V[1][1] - V[1][0] * V[0][1];
    const double sg = (cx * V[0][2] + cy * V[1][2] + cz * V[2][2]) < 0.0 ? -1.0 : 1.0;
    double* d = dir + (size_t)k * 9;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int r = 0; r < 3; r++) d[3 * j + r] = (j == 2 ? sg : 1.0) * V[r][j];
  }
}

// |s|^2 in the norm of the inverse small-strain moduli: dev(s):dev(s) / (2 mu) + tr(s)^2 / (9 K)
__device__ __forceinline__ double cinv_norm2(const double s[6], double i2mu, double i9K) {
  const double tr = s[0] + s[1] + s[2], m = tr * (1.0 / 3.0);
  const double d0 = s[0] - m, d1 = s[1] - m, d2 = s[2] - m;
  const double dd = d0 * d0 + d1 * d1 + d2 * d2 + 2.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]);
  return dd * i2mu + tr * tr * i9K;
}

// err [3][Epad] = eta_e^2 (clamped at 0) | n_e^2 | 1 where the sum was clamped.  MT as stress_point_kernel.
template <class MT>
__global__ __launch_bounds__(128) void zz_error_kernel(ElemView m, MT mat_in, RecoveryTable tb,
                                                      const double* __restrict__ pts, const double* __restrict__ nodal,
                                                      double* __restrict__ err) {
  __shared__ double tr_all[2 * 64 * kPtRow];
  double* tr = tr_all + (threadIdx.x >> 6) * (64 * kPtRow);  // this wavefront's slice
  const int lane = threadIdx.x & 63;
  const int e0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63);
  if (e0 >= m.E) return;  // the whole wavefront
  const int e_raw = e0 + lane;
  const int e = e_raw < m.E ? e_raw : m.E - 1;
  load_point_rows(pts, e0, m.E, lane, tr);
  const Material mat = mat_at(mat_in, e);
  const double mu = mat.model == kMooneyRivlin ? 2.0 * (mat.mu10 + mat.mu01) : mat.mu;
  const double K = mat.model == kMooneyRivlin ? mat.kappa : mat.lambda + (2.0 / 3.0) * mat.mu;
  const double i2mu = 1.0 / (2.0 * mu), i9K = 1.0 / (9.0 * K);
  // the recovered field at the rule's points, node by node in local order
  double eq[kNQ][6];
#pragma unroll
  for (int q = 0; q < kNQ; q++)
#pragma unroll
    for (int c = 0; c < 6; c++) eq[q][c] = 0.0;
#pragma unroll
  for (int a = 0; a < kNN; a++) {
    const double* r = nodal + (size_t)m.conn[(size_t)a * m.E + e] * 7;
    double sa[6];
#pragma unroll
    for (int c = 0; c < 6; c++) sa[c] = r[c];
#pragma unroll
    for (int q = 0; q < kNQ; q++)
#pragma unroll
      for (int c = 0; c < 6; c++) eq[q][c] += tb.Nq[q][a] * sa[c];
  }
  wave_sync();
  const double* row = tr + (e - e0) * kPtRow;
  double eta2 = 0.0, n2 = 0.0;
#pragma unroll
  for (int q = 0; q < kNQ; q++) {
    double sq[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
      sq[c] = row[q * 6 + c];
      eq[q][c] -= sq[c];
    }
    const double dV = m.detJ[(size_t)e * kNQ + q] * tb.qw[q];
    eta2 += dV * cinv_norm2(eq[q], i2mu, i9K);
    n2 += dV * cinv_norm2(sq, i2mu, i9K);
  }
  if (e_raw < m.E) {
    const bool clamped = eta2 < 0.0;
    err[(size_t)0 * m.Epad + e] = clamped ? 0.0 : eta2;
    err[(size_t)1 * m.Epad + e] = n2;
    err[(size_t)2 * m.Epad + e] = clamped ? 1.0 : 0.0;
  }
}

}  // namespace

void launch_recovery_elem(hipStream_t s, int E, const double* detJ, const RecoveryTable& tb, const double* pts, double* rec) {
  hipLaunchKernelGGL(recovery_elem_kernel, dim3((E + 127) / 128), dim3(128), 0, s, E, detJ, tb, pts, rec);
}

void launch_recovery_nodal(hipStream_t s, int N, const Incidence& inc, const double* rec, double* nodal) {
  hipLaunchKernelGGL(recovery_nodal_kernel, dim3((N + kNod - 1) / kNod), dim3(kNod), 0, s, N, inc, rec, nodal);
}

void launch_recovery_nodal_direct(hipStream_t s, int N, const Incidence& inc, const RecoveryTable& tb, const double* pts,
                                  const double* rec, double* nodal) {
  hipLaunchKernelGGL(recovery_nodal_direct_kernel, dim3((N + kNod - 1) / kNod), dim3(kNod), 0, s, N, inc, tb, pts, rec,
                     nodal);
}

void launch_principal(hipStream_t s, int n, const double* src, int stride, int offset, double* val, double* dir) {
  hipLaunchKernelGGL(principal_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, src, stride, offset, val, dir);
}

void launch_zz_error(hipStream_t s, const ElemView& m, const Material& mat, const double* emat, const RecoveryTable& tb,
                     const double* pts, const double* nodal, double* err) {
  const dim3 grid((m.E + 127) / 128), block(128);
  if (emat) hipLaunchKernelGGL((zz_error_kernel<MaterialPE>), grid, block, 0, s, m, MaterialPE{mat, emat}, tb, pts, nodal, err);
  else hipLaunchKernelGGL((zz_error_kernel<Material>), grid, block, 0, s, m, mat, tb, pts, nodal, err);
}

}  // namespace tlfea
