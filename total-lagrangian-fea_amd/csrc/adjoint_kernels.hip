// adjoint_kernels.hip -- adjoint sensitivities of the implicit Newton step (the ANCF kinds: 3j').
//
//   sens_point_kernel    thread per element (stress_point_kernel's lane mapping and reads: the coalesced element-fastest
//                        grad-N copy, next point's gradients in flight): F and the gradient D = grad w of the adjoint field
//                        at the five Keast points, the contraction -(dP/dtheta_p)(F) : D dV of every stiffness slot and the
//                        mass slot -(N w).(N u) dV; sens [P + 1][Epad], one coalesced store per slot.  P is linear in its
//                        stiffness parameters, so dP/dtheta_p needs no material value: the kernel takes the MODEL alone and
//                        one launch serves a uniform material and a per-element table alike (the table decides only which
//                        elements the reduction adds up)
//   adj_partial_kernel / adj_final_kernel
//                        fixed-order sums (stress_partial_kernel's scheme): a block adds a chunk of kAdjChunk consecutive
//                        items of one group in strided index order and a fixed tree, then one block per group adds the
//                        group's chunk sums the same way.  The chunks depend on the group sizes alone, never on a launch
//                        shape.  Groups: the ascending element list of every material (sens -> per_material), or all
//                        nodes (M w -> the three sums of a_bar)
//   ancf_sens_point_kernel / ancf_rho_terms_kernel
//                        the ANCF kinds (DESIGN 3j'): lanes own quadrature points; the density slot from M w and u
//   adj_rhs_kernel       thread per DOF: x_t = x_bar + rho J^T lam_bar, v_t = v_bar + h x_t, u = (v - v_prev)/h - a
//                        (a on the position coefficients: every coefficient of a T10 mesh, every fourth of an ANCF mesh)
//   adj_out_kernel       thread per DOF: f_ext_bar, v_prev_bar, x_prev_bar from w and M w; thread per constraint row:
//                        J w, lam_in_bar, t_bar
// J is the fixed-node selector (constraint 3 slot + c <-> component c of node fixed[slot]) or the CSR rows.
// No atomics: every launch is bitwise reproducible.
#include "elem_math.h"

namespace tlfea {
namespace {

constexpr int kRed = 256;  // threads of a reduction block

// (dP/dtheta_p)(F) : D for the stiffness parameters of the model: SVK (lambda, mu), Mooney-Rivlin (mu10, mu01, kappa);
// the same expressions as elastic_P with the parameter set to 1
template <int MODEL>
__device__ __forceinline__ void dP_contract(const double F[3][3], const double D[3][3], double s[3]) {
  double FD = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) FD += F[i][j] * D[i][j];
  if (MODEL == kMooneyRivlin) {
    MRState st;
    mr_state(F, 1.0, 1.0, 1.0, st);  // t1 = 2 J^-2/3, t2 = 2 J^-4/3, t3 = (J - 1) J
    double GD = 0.0, FCD = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        GD += st.G[i][j] * D[i][j];
        FCD += st.FC[i][j] * D[i][j];
      }
    s[0] = st.t1 * (FD - (st.I1 / 3.0) * GD);
    s[1] = st.t2 * (st.I1 * FD - FCD - (2.0 * st.I2 / 3.0) * GD);
    s[2] = st.t3 * GD;
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
    double FFtFD = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double fftf = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) fftf += FFt[i][k] * F[k][j];
        FFtFD += fftf * D[i][j];
      }
    s[0] = (0.5 * trFtF - 1.5) * FD;  // tr(E) F : D
    s[1] = FFtFD - FD;                // 2 F E : D
    s[2] = 0.0;
  }
}

// sens [P + 1][Epad], P = 2 (SVK) | 3 (Mooney-Rivlin): slots 0 .. P - 1 the stiffness parameters, slot P the density.
// w, u: [3N] interleaved; u null = no density slot wanted (zeros).
template <int MODEL>
__global__ __launch_bounds__(128) void sens_point_kernel(ElemView m, SensShape sh, const double* __restrict__ w,
                                                        const double* __restrict__ u, double* __restrict__ sens) {
  constexpr int S = kNN, Q = kNQ, P = MODEL == kMooneyRivlin ? 3 : 2;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m.E) return;  // nothing below crosses lanes
  int gn[S];
  double wn[S][3];
#pragma unroll
  for (int a = 0; a < S; a++) {
    gn[a] = m.conn[(size_t)a * m.E + e];
#pragma unroll
    for (int c = 0; c < 3; c++) wn[a][c] = w[3 * gn[a] + c];
  }
  double dV[Q];
#pragma unroll
  for (int q = 0; q < Q; q++) dV[q] = m.detJ[(size_t)e * Q + q] * m.qw[q];
  // density slot first: u is needed here only, so its 30 registers are free again before the gradients arrive
  double am = 0.0;
  if (u != nullptr) {
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
          Nw[q][c] += sh.Nq[q][a] * wn[a][c];
          Nu[q][c] += sh.Nq[q][a] * ua[c];
        }
    }
#pragma unroll
    for (int q = 0; q < Q; q++) am += dV[q] * (Nw[q][0] * Nu[q][0] + Nw[q][1] * Nu[q][1] + Nw[q][2] * Nu[q][2]);
  }
  double xn[S][3];
#pragma unroll
  for (int a = 0; a < S; a++) {
    xn[a][0] = m.x[gn[a]];
    xn[a][1] = m.y[gn[a]];
    xn[a][2] = m.z[gn[a]];
  }
  double acc[3] = {0.0, 0.0, 0.0};
  // as stress_point_kernel: the next point's gradients are in flight while this point computes
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
    double s[3];
    dP_contract<MODEL>(F, D, s);
    const double dv = q == 0 ? dV[0] : (q == 1 ? dV[1] : (q == 2 ? dV[2] : (q == 3 ? dV[3] : dV[4])));
#pragma unroll
    for (int p = 0; p < P; p++) acc[p] += s[p] * dv;
  }
#pragma unroll
  for (int p = 0; p < P; p++) sens[(size_t)p * m.Epad + e] = -acc[p];
  sens[(size_t)P * m.Epad + e] = -am;
}

// The ANCF kinds (DESIGN 3j'): lanes own quadrature points, the mapping of ancf_stress_point_kernel (3f').  A wavefront
// takes G = 64 / Q elements of Q lanes each (shell <16,48>: 1 x 48, beam <8,12>: 5 x 12); the elements' coefficient vectors x
// and the adjoint field w sit in the wavefront's LDS slice (3 S + 1 doubles per element each: the G rows start on different
// banks) and are read as broadcasts; every lane streams its own contiguous 3 S gradient doubles of gradN [E][Q][3][S] once,
// into F and D = sum_a w_a (x) grad s_a alike, and forms the P contractions of its point.  The element sums are
// elem_lane_sum's fixed tree; lanes past the wavefront's last element recompute element e0 with dV = 0.  The four
// wavefronts of a block share nothing.  sens [P][Epad]: stiffness slots only (the density slot of an ANCF object is a
// vector product, ancf_rho_terms_kernel).
template <int S, int Q, int MODEL>
__global__ __launch_bounds__(64 * kAncfWaves) void ancf_sens_point_kernel(ElemView m, const double* __restrict__ w,
                                                                         double* __restrict__ sens) {
  constexpr int G = 64 / Q, kRow = 3 * S + 1, P = MODEL == kMooneyRivlin ? 3 : 2;
  __shared__ double xs_all[kAncfWaves][G * kRow], ws_all[kAncfWaves][G * kRow];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e0 = (blockIdx.x * kAncfWaves + wv) * G;  // first element of this wavefront
  if (e0 >= m.E) return;                              // the whole wavefront: nothing below synchronises across wavefronts
  double *xs = xs_all[wv], *ws = ws_all[wv];
  const int n_el = min(G, m.E - e0);
  for (int idx = lane; idx < n_el * S; idx += 64) {
    const int el = idx / S, a = idx - el * S;
    const int c = m.conn[(size_t)a * m.E + e0 + el];
    double* xo = xs + el * kRow + 3 * a;
    xo[0] = m.x[c];
    xo[1] = m.y[c];
    xo[2] = m.z[c];
    double* wo = ws + el * kRow + 3 * a;
    wo[0] = w[3 * (size_t)c];
    wo[1] = w[3 * (size_t)c + 1];
    wo[2] = w[3 * (size_t)c + 2];
  }
  wave_sync();
  const int g_raw = lane / Q, p = lane - g_raw * Q;
  const bool active = g_raw < n_el;
  const int g = active ? g_raw : 0, e = e0 + g;
  const double2* gr = reinterpret_cast<const double2*>(m.gradN + ((size_t)e * Q + p) * (3 * S));  // 3 S doubles: 16-byte aligned
  const double* xe = xs + g * kRow;
  const double* we = ws + g * kRow;
  double F[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, D[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
  for (int d = 0; d < 3; d++)
#pragma unroll
    for (int a = 0; a < S; a += 2) {
      const double2 h = gr[(d * S + a) >> 1];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        F[i][d] += xe[3 * a + i] * h.x + xe[3 * a + 3 + i] * h.y;
        D[i][d] += we[3 * a + i] * h.x + we[3 * a + 3 + i] * h.y;
      }
    }
  double s[3];
  dP_contract<MODEL>(F, D, s);
  const double dV = active ? m.detJ[(size_t)e * Q + p] * m.qw[p] : 0.0;
#pragma unroll
  for (int k = 0; k < P; k++) {
    const double acc = elem_lane_sum<Q>(s[k] * dV, lane, p);
    if (active && p == 0) sens[(size_t)k * m.Epad + e] = -acc;
  }
}

// The density slot of an ANCF object, whose mass matrix is linear in its one density: item i = scale (M w)_i . u_i per
// coefficient vector (scale = -1 / rho0 of the assembled matrix); adj_partial / adj_final add the items up
__global__ __launch_bounds__(256) void ancf_rho_terms_kernel(int N, const double* __restrict__ Mw, const double* __restrict__ u,
                                                            double scale, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t k = 3 * (size_t)i;
  out[i] = scale * (Mw[k] * u[k] + Mw[k + 1] * u[k + 1] + Mw[k + 2] * u[k + 2]);
}

// value (slot c, item k) = src[c * slot_stride + item * item_stride], item = idx ? idx[k] : k.  Block b adds the items
// [blk[b].x, blk[b].y) (blk null: [b kAdjChunk, min(n, (b + 1) kAdjChunk))); partial [blocks][SLOTS].
template <int SLOTS>
__global__ __launch_bounds__(kRed) void adj_partial_kernel(int n, const int2* __restrict__ blk, const int* __restrict__ idx,
                                                          const double* __restrict__ src, size_t slot_stride,
                                                          int item_stride, double* __restrict__ partial) {
  __shared__ double acc[SLOTS][kRed];
  const int b = blockIdx.x, t = threadIdx.x;
  const int k0 = blk ? blk[b].x : b * kAdjChunk, k1 = blk ? blk[b].y : min(n, (b + 1) * kAdjChunk);
  double a[SLOTS];
#pragma unroll
  for (int c = 0; c < SLOTS; c++) a[c] = 0.0;
  for (int k = k0 + t; k < k1; k += kRed) {
    const size_t item = (size_t)(idx ? idx[k] : k) * item_stride;
#pragma unroll
    for (int c = 0; c < SLOTS; c++) a[c] += src[(size_t)c * slot_stride + item];
  }
#pragma unroll
  for (int c = 0; c < SLOTS; c++) acc[c][t] = a[c];
  __syncthreads();
  for (int s = kRed / 2; s > 0; s >>= 1) {
    if (t < s)
#pragma unroll
      for (int c = 0; c < SLOTS; c++) acc[c][t] += acc[c][t + s];
    __syncthreads();
  }
  if (t < SLOTS) partial[(size_t)b * SLOTS + t] = acc[t][0];
}

// out [groups][SLOTS]: block g adds the partial rows [boff[g], boff[g + 1]) (boff null: one group, rows [0, nb))
template <int SLOTS>
__global__ __launch_bounds__(kRed) void adj_final_kernel(const int* __restrict__ boff, int nb,
                                                        const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double acc[SLOTS][kRed];
  const int g = blockIdx.x, t = threadIdx.x;
  const int b0 = boff ? boff[g] : 0, b1 = boff ? boff[g + 1] : nb;
  double a[SLOTS];
#pragma unroll
  for (int c = 0; c < SLOTS; c++) a[c] = 0.0;
  for (int b = b0 + t; b < b1; b += kRed)
#pragma unroll
    for (int c = 0; c < SLOTS; c++) a[c] += partial[(size_t)b * SLOTS + c];
#pragma unroll
  for (int c = 0; c < SLOTS; c++) acc[c][t] = a[c];
  __syncthreads();
  for (int s = kRed / 2; s > 0; s >>= 1) {
    if (t < s)
#pragma unroll
      for (int c = 0; c < SLOTS; c++) acc[c][t] += acc[c][t + s];
    __syncthreads();
  }
  if (t < SLOTS) out[(size_t)g * SLOTS + t] = acc[t][0];
}

// sum_r J^T[i][r] lam[r] of DOF i (lam null: 0)
__device__ __forceinline__ double jt_times(const AdjCons& J, int i, const double* __restrict__ lam) {
  if (lam == nullptr) return 0.0;
  if (J.mode == 1) {
    const int n = i / 3, slot = J.fixed_slot[n];
    return slot >= 0 ? lam[3 * slot + (i - 3 * n)] : 0.0;
  }
  if (J.mode != 2) return 0.0;
  double s = 0.0;
  for (int k = J.jtoff[i]; k < J.jtoff[i + 1]; k++) s += J.jtval[k] * lam[J.jtcol[k]];  // ascending constraint id
  return s;
}

__global__ __launch_bounds__(256) void adj_rhs_kernel(int n, AdjCons J, const double* __restrict__ xbar,
                                                     const double* __restrict__ vbar, const double* __restrict__ lambar,
                                                     const double* __restrict__ v, const double* __restrict__ vprev,
                                                     double ax, double ay, double az, int stride, double h,
                                                     double rho, double* __restrict__ xt, double* __restrict__ vt,
                                                     double* __restrict__ u) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = (xbar ? xbar[i] : 0.0) + rho * jt_times(J, i, lambar);
  xt[i] = x;
  vt[i] = (vbar ? vbar[i] : 0.0) + h * x;
  const int c = i % 3;
  const double a = (i / 3) % stride ? 0.0 : (c == 0 ? ax : (c == 1 ? ay : az));  // a gradient coefficient: a_i = 0 (body_force_kernel)
  u[i] = (v[i] - vprev[i]) / h - a;
}

__global__ __launch_bounds__(256) void adj_out_kernel(int n, int nc, AdjCons J, const double* __restrict__ w,
                                                     const double* __restrict__ Mw, const double* __restrict__ xt,
                                                     const double* __restrict__ vt, const double* __restrict__ lambar,
                                                     double h, double rho, double* __restrict__ fext_bar,
                                                     double* __restrict__ vprev_bar, double* __restrict__ xprev_bar,
                                                     double* __restrict__ lam_in_bar, double* __restrict__ t_bar) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const double mh = Mw[i] / h;
    if (fext_bar) fext_bar[i] = w[i];
    if (vprev_bar) vprev_bar[i] = mh;
    if (xprev_bar) xprev_bar[i] = xt[i] - (vt[i] - mh) / h;  // dg/dx_prev = (H - M/h) / h: no stiffness product
    return;
  }
  const int r = i - n;
  if (r >= nc) return;
  double Jw = 0.0;
  if (J.mode == 1) {
    Jw = w[3 * J.fixed[r / 3] + r % 3];
  } else {
    for (int k = J.joff[r]; k < J.joff[r + 1]; k++) Jw += J.jval[k] * w[J.jcol[k]];
  }
  const double lb = lambar ? lambar[r] : 0.0;
  if (lam_in_bar) lam_in_bar[r] = lb - h * Jw;
  if (t_bar) t_bar[r] = h * rho * Jw - rho * lb;
}

// out [E][slots] from the plane-major sens [slots][Epad]
__global__ __launch_bounds__(256) void sens_transpose_kernel(int E, int Epad, int slots, const double* __restrict__ sens,
                                                            double* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= (size_t)E * slots) return;
  const size_t e = k / slots, c = k - e * slots;
  out[k] = sens[c * Epad + e];
}

template <int SLOTS>
void launch_sums_t(hipStream_t s, int n, int nb, const int2* blk, const int* idx, const double* src, size_t slot_stride,
                   int item_stride, int groups, const int* boff, double* partial, double* out) {
  hipLaunchKernelGGL(adj_partial_kernel<SLOTS>, dim3(nb), dim3(kRed), 0, s, n, blk, idx, src, slot_stride, item_stride,
                     partial);
  hipLaunchKernelGGL(adj_final_kernel<SLOTS>, dim3(groups), dim3(kRed), 0, s, boff, nb, partial, out);
}

}  // namespace

void launch_sens_points(hipStream_t s, const ElemView& m, int model, const SensShape& sh, const double* w, const double* u,
                        double* sens) {
  const dim3 grid((m.E + 127) / 128), block(128);
  if (model == kMooneyRivlin)
    hipLaunchKernelGGL(sens_point_kernel<kMooneyRivlin>, grid, block, 0, s, m, sh, w, u, sens);
  else
    hipLaunchKernelGGL(sens_point_kernel<kSVK>, grid, block, 0, s, m, sh, w, u, sens);
}

template <int S, int Q>
static void launch_ancf_sens_t(hipStream_t s, const ElemView& m, int model, const double* w, double* sens) {
  constexpr int G = 64 / Q;
  const dim3 grid((m.E + kAncfWaves * G - 1) / (kAncfWaves * G)), block(64 * kAncfWaves);
  if (model == kMooneyRivlin)
    hipLaunchKernelGGL((ancf_sens_point_kernel<S, Q, kMooneyRivlin>), grid, block, 0, s, m, w, sens);
  else
    hipLaunchKernelGGL((ancf_sens_point_kernel<S, Q, kSVK>), grid, block, 0, s, m, w, sens);
}

void launch_ancf_sens_points(hipStream_t s, const ElemView& m, int model, const double* w, double* sens) {
  if (m.S == 8) launch_ancf_sens_t<8, 12>(s, m, model, w, sens);
  else launch_ancf_sens_t<16, 48>(s, m, model, w, sens);
}

void launch_ancf_rho_terms(hipStream_t s, int N, const double* Mw, const double* u, double scale, double* out) {
  hipLaunchKernelGGL(ancf_rho_terms_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, Mw, u, scale, out);
}

void launch_sens_transpose(hipStream_t s, int E, int Epad, int slots, const double* sens, double* out) {
  const size_t n = (size_t)E * slots;
  hipLaunchKernelGGL(sens_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, E, Epad, slots, sens, out);
}

void launch_adj_sums(hipStream_t s, int slots, int n, int nb, const int2* blk, const int* idx, const double* src,
                     size_t slot_stride, int item_stride, int groups, const int* boff, double* partial, double* out) {
  if (slots == 4) launch_sums_t<4>(s, n, nb, blk, idx, src, slot_stride, item_stride, groups, boff, partial, out);
  else if (slots == 2) launch_sums_t<2>(s, n, nb, blk, idx, src, slot_stride, item_stride, groups, boff, partial, out);
  else if (slots == 1) launch_sums_t<1>(s, n, nb, blk, idx, src, slot_stride, item_stride, groups, boff, partial, out);
  else launch_sums_t<3>(s, n, nb, blk, idx, src, slot_stride, item_stride, groups, boff, partial, out);
}

void launch_adj_rhs(hipStream_t s, int n, const AdjCons& J, const double* xbar, const double* vbar, const double* lambar,
                    const double* v, const double* vprev, const double a[3], int stride, double h, double rho, double* xt,
                    double* vt, double* u) {
  hipLaunchKernelGGL(adj_rhs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, J, xbar, vbar, lambar, v, vprev, a[0],
                     a[1], a[2], stride, h, rho, xt, vt, u);
}

void launch_adj_out(hipStream_t s, int n, int nc, const AdjCons& J, const double* w, const double* Mw, const double* xt,
                    const double* vt, const double* lambar, double h, double rho, double* fext_bar, double* vprev_bar,
                    double* xprev_bar, double* lam_in_bar, double* t_bar) {
  const int total = n + (J.mode ? nc : 0);
  hipLaunchKernelGGL(adj_out_kernel, dim3((total + 255) / 256), dim3(256), 0, s, n, J.mode ? nc : 0, J, w, Mw, xt, vt,
                     lambar, h, rho, fext_bar, vprev_bar, xprev_bar, lam_in_bar, t_bar);
}

}  // namespace tlfea
