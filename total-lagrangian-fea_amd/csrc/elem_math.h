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

}  // namespace tlfea
