// elem_math.h -- device-side 3x3 helpers, the constitutive laws and the wave-level LDS hand-off shared by the element
// kernels (elem_kernels.hip) and the stress recovery (stress_kernels.hip).  Everything is __forceinline__: each
// translation unit compiles its own copy into its kernels.
#pragma once
#include "tlfea_internal.h"

namespace tlfea {

// ------------------------------------------------------------------------------------------------
// small 3x3 helpers (registers only)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double det3(const double A[3][3]) {
  return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
         A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// inverse-transpose with the reference's determinant clamp (MooneyRivlin.cuh:25-43)
__device__ __forceinline__ void inv_transpose3(const double A[3][3], double detA, double G[3][3]) {
  const double eps = 1e-12;
  double sd = detA;
  if (fabs(sd) < eps) sd = (sd >= 0.0) ? eps : -eps;
  const double id = 1.0 / sd;
  G[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) * id;
  G[0][1] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) * id;
  G[0][2] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) * id;
  G[1][0] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * id;
  G[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * id;
  G[1][2] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * id;
  G[2][0] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * id;
  G[2][1] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * id;
  G[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * id;
}

// Invariants and helper matrices of compressible Mooney-Rivlin (MooneyRivlin.cuh:48-95).
struct MRState {
  double C[3][3], FC[3][3], FFT[3][3], G[3][3];  // G = F^-T
  double I1, I2, J, t1, t2, t3;
};

__device__ __forceinline__ void mr_state(const double F[3][3], double mu10, double mu01, double kappa, MRState& s) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double c = 0.0, b = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        c += F[k][i] * F[k][j];
        b += F[i][k] * F[j][k];
      }
      s.C[i][j] = c;
      s.FFT[i][j] = b;
    }
  s.I1 = s.C[0][0] + s.C[1][1] + s.C[2][2];
  double trC2 = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) trC2 += s.C[i][k] * s.C[k][i];
  s.I2 = 0.5 * (s.I1 * s.I1 - trC2);
  s.J = det3(F);
  inv_transpose3(F, s.J, s.G);
  const double J13 = cbrt(s.J);
  const double Jm23 = 1.0 / (J13 * J13);
  const double Jm43 = Jm23 * Jm23;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++) v += F[i][k] * s.C[k][j];
      s.FC[i][j] = v;
    }
  s.t1 = 2.0 * mu10 * Jm23;
  s.t2 = 2.0 * mu01 * Jm43;
  s.t3 = kappa * (s.J - 1.0) * s.J;
}

// First Piola-Kirchhoff stress.  SVK: SVK.cuh:14-32;  MR: MooneyRivlin.cuh:45-111.
__device__ __forceinline__ void elastic_P(const double F[3][3], const Material& mat, double P[3][3]) {
  if (mat.model == kMooneyRivlin) {
    MRState s;
    mr_state(F, mat.mu10, mat.mu01, mat.kappa, s);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double term1 = F[i][j] - (s.I1 / 3.0) * s.G[i][j];
        const double term2 = s.I1 * F[i][j] - s.FC[i][j] - (2.0 * s.I2 / 3.0) * s.G[i][j];
        P[i][j] = s.t1 * term1 + s.t2 * term2 + s.t3 * s.G[i][j];
      }
  } else {
    double FFt[3][3], trFtF = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double b = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) b += F[i][k] * F[j][k];
        FFt[i][j] = b;
        trFtF += F[i][j] * F[i][j];
      }
    const double lf = mat.lambda * (0.5 * trFtF - 1.5);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double fftf = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) fftf += FFt[i][k] * F[k][j];
        P[i][j] = lf * F[i][j] + mat.mu * (fftf - F[i][j]);
      }
  }
}

// Material tangent of elastic_P applied to D: dP = (dP/dF) : D (shape sensitivities).
// SVK: D S2 + F (lambda tr(dE) I + 2 mu dE), dE = sym(F^T D), S2 = lambda tr(E) I + 2 mu E.
// MR, term by term of elastic_P with g = G : D (dJ = J g), dI1 = 2 F : D, dC = F^T D + D^T F, dI2 = I1 dI1 - tr(C dC),
// dG = -G D^T G.
__device__ __forceinline__ void elastic_dP(const double F[3][3], const double D[3][3], const Material& mat, double dP[3][3]) {
  double FD = 0.0, FtD[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++) a += F[k][i] * D[k][j];
      FtD[i][j] = a;
      FD += F[i][j] * D[i][j];
    }
  if (mat.model == kMooneyRivlin) {
    MRState s;
    mr_state(F, mat.mu10, mat.mu01, mat.kappa, s);
    double g = 0.0, CdC = 0.0, dG[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        g += s.G[i][j] * D[i][j];
        CdC += s.C[i][j] * (FtD[i][j] + FtD[j][i]);  // C and dC are symmetric: tr(C dC) = C : dC
      }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double a = 0.0;  // (G D^T G)_ij = sum_kl G_ik D_lk G_lj
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
          for (int l = 0; l < 3; l++) a += s.G[i][k] * D[l][k] * s.G[l][j];
        dG[i][j] = -a;
      }
    const double dI1 = 2.0 * FD, dI2 = s.I1 * dI1 - CdC;
    const double t3d = mat.kappa * (2.0 * s.J - 1.0) * s.J * g;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double DC = 0.0, FdC = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          DC += D[i][k] * s.C[k][j];
          FdC += F[i][k] * (FtD[k][j] + FtD[j][k]);
        }
        const double term1 = F[i][j] - (s.I1 / 3.0) * s.G[i][j];
        const double term2 = s.I1 * F[i][j] - s.FC[i][j] - (2.0 * s.I2 / 3.0) * s.G[i][j];
        const double d1 = -(2.0 / 3.0) * g * term1 + D[i][j] - (dI1 / 3.0) * s.G[i][j] - (s.I1 / 3.0) * dG[i][j];
        const double d2 = -(4.0 / 3.0) * g * term2 + dI1 * F[i][j] + s.I1 * D[i][j] - DC - FdC -
                          (2.0 * dI2 / 3.0) * s.G[i][j] - (2.0 * s.I2 / 3.0) * dG[i][j];
        dP[i][j] = s.t1 * d1 + s.t2 * d2 + t3d * s.G[i][j] + s.t3 * dG[i][j];
      }
  } else {
    double C[3][3], trC = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) c += F[k][i] * F[k][j];
        C[i][j] = c;
      }
    trC = C[0][0] + C[1][1] + C[2][2];
    const double ltrE = mat.lambda * (0.5 * trC - 1.5), ltrdE = mat.lambda * FD;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double DC = 0.0, FdE2 = 0.0;  // D C, F (F^T D + D^T F) = 2 F dE
#pragma unroll
        for (int k = 0; k < 3; k++) {
          DC += D[i][k] * C[k][j];
          FdE2 += F[i][k] * (FtD[k][j] + FtD[j][k]);
        }
        dP[i][j] = ltrE * D[i][j] + mat.mu * (DC - D[i][j]) + ltrdE * F[i][j] + mat.mu * FdE2;
      }
  }
}

// Wave-private LDS hand-offs (the fused assembly kernels' workgroup is ONE wavefront; the residual launch transposes its
// stores inside each wavefront's own slice): a wavefront's LDS instructions execute in program order, so data written by one
// lane is visible to the lanes of every later LDS instruction without a barrier.  What remains of __syncthreads() is the
// compiler-level ordering -- and NOT its s_waitcnt vmcnt(0), which would drain the prefetched index loads and the H row
// stores at every one of the 3-5 synchronisation points of a pass.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- lanes own quadrature points (the ANCF kinds: stress_kernels.hip, adjoint_kernels.hip; DESIGN 3f') -----------------
constexpr int kAncfWaves = 4;  // wavefronts of a block; each works on its own elements through its own LDS slice
// sum of `val` over the Q lanes of an element, valid in the element's lane 0 (p = lane within the element).  Every lane
// of the wavefront takes part in every shuffle; the shape depends on Q alone, so a launch is bitwise reproducible.
template <int Q>
__device__ __forceinline__ double elem_lane_sum(double val, int lane, int p) {
  static_assert(Q % 3 == 0 && ((Q / 3) & (Q / 3 - 1)) == 0, "Q = 3 * 2^k");
#pragma unroll
  for (int off = Q / 2; off >= 3; off >>= 1) {
    const double t = __shfl(val, (lane + off) & 63);
    if (p < off) val += t;
  }
  const double t1 = __shfl(val, (lane + 1) & 63), t2 = __shfl(val, (lane + 2) & 63);
  return (val + t1) + t2;
}

}  // namespace tlfea
