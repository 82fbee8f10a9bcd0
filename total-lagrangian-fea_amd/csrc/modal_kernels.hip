// modal_kernels.hip -- block-vector kernels of the modal solve (LOBPCG).
//
// A block vector holds `ld` doubles per DOF row, the columns of one DOF contiguous: X[(3 node + c) ld + j].  One gather
// of a neighbour node therefore brings 3 ld contiguous doubles, and a lane group reads a DOF row coalesced.  Every sum
// below runs in a fixed order (ascending CSR column, ascending row inside a slab, ascending slab), nothing is
// accumulated with atomics: all results are bitwise reproducible run to run.
#include "tlfea_internal.h"

#include <algorithm>

namespace tlfea {

// ---- Y = H X (3 x 3 block CSR) and Y = (M (x) I3) X (node-level mass CSR) ---------------------------------------
// G = 4 .. 32 lanes (the power of two >= m) own one node row, a wavefront 64 / G rows at a time; lane j of the group owns
// column j and keeps the row's three components in registers, so a neighbour's X row is gathered once per column and a
// matrix block is fetched once per lane group (one address for all its lanes) and reused by every column.  Neighbours
// are added in ascending CSR order by every lane for itself: no cross-lane sum, no atomics.
template <bool MASS>
__global__ __launch_bounds__(256) void spmm_block_kernel(int N, int m, int G, const int* __restrict__ off,
                                                         const int* __restrict__ cols, const double* __restrict__ val,
                                                         const double* __restrict__ X, int ldx, double* __restrict__ Y,
                                                         int ldy, const int* __restrict__ fixed_slot) {
  const int rows_per_block = 256 / G;
  const int j = threadIdx.x % G, g = threadIdx.x / G;
  for (int i = blockIdx.x * rows_per_block + g; i < N; i += gridDim.x * rows_per_block) {
    if (j >= m) continue;
    const int o0 = off[i], deg = off[i + 1] - o0;
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    if (MASS) {
      for (int k = 0; k < deg; k++) {
        const double mv = val[o0 + k];
        const double* x = X + (size_t)3 * cols[o0 + k] * ldx + j;
        y0 += mv * x[0];
        y1 += mv * x[ldx];
        y2 += mv * x[2 * ldx];
      }
    } else {
      const double* Hi = val + (size_t)9 * o0;   // row component d of the node row: Hi[d * 3 deg + 3 k + e]
      const int row = 3 * deg;
      for (int k = 0; k < deg; k++) {
        const double* x = X + (size_t)3 * cols[o0 + k] * ldx + j;
        const double x0 = x[0], x1 = x[ldx], x2 = x[2 * ldx];
        const double* h = Hi + 3 * k;
        y0 += h[0] * x0 + h[1] * x1 + h[2] * x2;
        y1 += h[row] * x0 + h[row + 1] * x1 + h[row + 2] * x2;
        y2 += h[2 * row] * x0 + h[2 * row + 1] * x1 + h[2 * row + 2] * x2;
      }
    }
    if (fixed_slot && fixed_slot[i] >= 0) y0 = y1 = y2 = 0.0;   // pinned rows of a block vector stay zero
    double* y = Y + (size_t)3 * i * ldy + j;
    y[0] = y0;
    y[ldy] = y1;
    y[2 * ldy] = y2;
  }
}

static int group_lanes(int m) {
  int G = 4;
  while (G < m) G *= 2;
  return G;
}

void launch_spmm_block(hipStream_t s, int N, int m, const int* off, const int* cols, const double* Hval, const double* X,
                       int ldx, double* Y, int ldy, const int* fixed_slot) {
  const int G = group_lanes(m), rpb = 256 / G;
  const int grid = std::max(1, std::min(4096, (N + rpb - 1) / rpb));
  hipLaunchKernelGGL(spmm_block_kernel<false>, dim3(grid), dim3(256), 0, s, N, m, G, off, cols, Hval, X, ldx, Y, ldy,
                     fixed_slot);
}

void launch_massmm_block(hipStream_t s, int N, int m, const int* off, const int* cols, const double* mval, const double* X,
                         int ldx, double* Y, int ldy, const int* fixed_slot) {
  const int G = group_lanes(m), rpb = 256 / G;
  const int grid = std::max(1, std::min(4096, (N + rpb - 1) / rpb));
  hipLaunchKernelGGL(spmm_block_kernel<true>, dim3(grid), dim3(256), 0, s, N, m, G, off, cols, mval, X, ldx, Y, ldy,
                     fixed_slot);
}

// ---- G = X^T Y, p, q <= 96 --------------------------------------------------------------------------------------
// Slab b = rows [b rows_per_slab, (b + 1) rows_per_slab) goes to workgroup b, which writes the slab's p x q sums into its
// own slot.  16 rows at a time are staged in LDS (zero-padded to 96 columns); thread (ty, tx) of the 16 x 16 workgroup
// owns entries (ty + 16 a, tx + 16 b), a, b < 6, in registers and adds the rows in ascending order.  gram_reduce_kernel
// then adds the slots in ascending slab order.  The slab size depends on the row count alone, so two calls -- and two
// solver objects on the same mesh -- form the same sums.  VALU only: the Gram products are a few percent of an iteration
// next to the per-column preconditioner, so the v_mfma_f64_16x16x4 form was not built.
constexpr int kGramMax = 96, kGramRows = 16, kGramSlabsMax = 512;  // two slabs per CU once the block has 131 072 rows

__global__ __launch_bounds__(256) void gram_kernel(int n, int rows_per_slab, int p, int q, const double* __restrict__ X,
                                                   int ldx, const double* __restrict__ Y, int ldy,
                                                   double* __restrict__ slots) {
  __shared__ double Xs[kGramRows][kGramMax];
  __shared__ double Ys[kGramRows][kGramMax];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[6][6];
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++) acc[a][b] = 0.0;
  const int r0 = blockIdx.x * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
  for (int rb = r0; rb < r1; rb += kGramRows) {
    for (int t = threadIdx.x; t < kGramRows * kGramMax; t += 256) {
      const int r = t / kGramMax, c = t - r * kGramMax;
      const bool in = rb + r < r1;
      Xs[r][c] = (in && c < p) ? X[(size_t)(rb + r) * ldx + c] : 0.0;
      Ys[r][c] = (in && c < q) ? Y[(size_t)(rb + r) * ldy + c] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < kGramRows; r++) {
      double xa[6], yb[6];
#pragma unroll
      for (int a = 0; a < 6; a++) xa[a] = Xs[r][ty + 16 * a];
#pragma unroll
      for (int b = 0; b < 6; b++) yb[b] = Ys[r][tx + 16 * b];
#pragma unroll
      for (int a = 0; a < 6; a++)
        if (16 * a < p) {
#pragma unroll
          for (int b = 0; b < 6; b++)
            if (16 * b < q) acc[a][b] += xa[a] * yb[b];
        }
    }
    __syncthreads();
  }
  double* out = slots + (size_t)blockIdx.x * p * q;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b < 6; b++) {
      const int i = ty + 16 * a, j = tx + 16 * b;
      if (i < p && j < q) out[i * q + j] = acc[a][b];
    }
}

// out[e] = sum over slots b = 0 .. n_slots - 1 (ascending) of slots[b][e]
__global__ __launch_bounds__(256) void gram_reduce_kernel(int n_slots, int count, const double* __restrict__ slots,
                                                          double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double s = 0.0;
  for (int b = 0; b < n_slots; b++) s += slots[(size_t)b * count + e];
  out[e] = s;
}

static int gram_rows_per_slab(int n) { return std::max(256, (n + kGramSlabsMax - 1) / kGramSlabsMax); }
// doubles of the slot buffer a launch_gram of p x q (or a launch_block_residual of 2 m <= p q) over n rows needs
size_t gram_slot_doubles(int n, int p, int q) {
  const int rps = gram_rows_per_slab(n);
  return (size_t)((n + rps - 1) / rps) * p * q;
}

void launch_gram(hipStream_t s, int n, int p, int q, const double* X, int ldx, const double* Y, int ldy, double* slots,
                 double* G) {
  const int rows_per_slab = gram_rows_per_slab(n);
  const int nb = (n + rows_per_slab - 1) / rows_per_slab;
  hipLaunchKernelGGL(gram_kernel, dim3(nb), dim3(256), 0, s, n, rows_per_slab, p, q, X, ldx, Y, ldy, slots);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((p * q + 255) / 256), dim3(256), 0, s, nb, p * q, slots, G);
}

// ---- Z = S C: new columns of a block from its old ones ------------------------------------------------------------
// One thread per DOF row: the row's k = k_end old columns go to registers first, then the nz new ones are written, the
// first nz0 at column z0, the rest at column z1 -- so X and P are replaced in place in one pass (a row depends on
// nothing but itself).  C [k][nz] is the small host-made matrix; every lane reads the same entry.
__global__ __launch_bounds__(128) void block_combine_kernel(int n, int k, double* __restrict__ S, int ld,
                                                            const double* __restrict__ C, int nz, int nz0, int z0, int z1) {
  const int r = blockIdx.x * 128 + threadIdx.x;
  if (r >= n) return;
  double* row = S + (size_t)r * ld;
  double v[kGramMax];
#pragma unroll
  for (int i = 0; i < kGramMax; i++) v[i] = i < k ? row[i] : 0.0;
  for (int j = 0; j < nz; j++) {
    double z = 0.0;
#pragma unroll
    for (int i = 0; i < kGramMax; i++)   // unrolled over the cap: v stays in registers; i < k is uniform
      if (i < k) z += v[i] * C[i * nz + j];
    row[j < nz0 ? z0 + j : z1 + (j - nz0)] = z;
  }
}

void launch_block_combine(hipStream_t s, int n, int k, double* S, int ld, const double* C, int nz, int nz0, int z0, int z1) {
  hipLaunchKernelGGL(block_combine_kernel, dim3((n + 127) / 128), dim3(128), 0, s, n, k, S, ld, C, nz, nz0, z0, z1);
}

// ---- R = AX - MX diag(mu), with the squared column norms of R and MX ---------------------------------------------
// Workgroup b takes slab b (as in gram_kernel); lane (t & 31) owns column j, the 8 lane rows of the workgroup take
// every 8th row of the slab in ascending order, and their 8 partial sums are added in ascending lane-row order.
// Slot b holds [m] |r|^2 then [m] |Mx|^2; gram_reduce_kernel adds the slots.
__global__ __launch_bounds__(256) void block_residual_kernel(int n, int rows_per_slab, int m,
                                                             const double* __restrict__ AX, const double* __restrict__ MX,
                                                             int ld, const double* __restrict__ mu, double* __restrict__ R,
                                                             int ldr, double* __restrict__ slots) {
  __shared__ double sh[2][8][32];
  const int j = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int r0 = blockIdx.x * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
  double rr = 0.0, mm = 0.0;
  if (j < m) {
    const double mj = mu[j];
    for (int r = r0 + g; r < r1; r += 8) {
      const double mx = MX[(size_t)r * ld + j];
      const double v = AX[(size_t)r * ld + j] - mj * mx;
      R[(size_t)r * ldr + j] = v;
      rr += v * v;
      mm += mx * mx;
    }
  }
  sh[0][g][j] = rr;
  sh[1][g][j] = mm;
  __syncthreads();
  if (g == 0 && j < m) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < 8; k++) {
      a += sh[0][k][j];
      b += sh[1][k][j];
    }
    slots[(size_t)blockIdx.x * 2 * m + j] = a;
    slots[(size_t)blockIdx.x * 2 * m + m + j] = b;
  }
}

void launch_block_residual(hipStream_t s, int n, int m, const double* AX, const double* MX, int ld, const double* mu,
                           double* R, int ldr, double* slots, double* norms2) {
  const int rows_per_slab = gram_rows_per_slab(n);
  const int nb = (n + rows_per_slab - 1) / rows_per_slab;
  hipLaunchKernelGGL(block_residual_kernel, dim3(nb), dim3(256), 0, s, n, rows_per_slab, m, AX, MX, ld, mu, R, ldr, slots);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(1), dim3(256), 0, s, nb, 2 * m, slots, norms2);
}

// ---- columns in and out of a block, the start block ----------------------------------------------------------------
__global__ void block_get_col_kernel(int n, const double* __restrict__ B, int ld, int j, double* __restrict__ v) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) v[r] = B[(size_t)r * ld + j];
}
// B[:, j] = v (zero where v is null), zero on pinned rows
__global__ void block_set_col_kernel(int n, const double* __restrict__ v, const int* __restrict__ fixed_slot,
                                     double* __restrict__ B, int ld, int j) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const bool pinned = fixed_slot && fixed_slot[r / 3] >= 0;
  B[(size_t)r * ld + j] = (v && !pinned) ? v[r] : 0.0;
}
void launch_block_get_col(hipStream_t s, int n, const double* B, int ld, int j, double* v) {
  hipLaunchKernelGGL(block_get_col_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, B, ld, j, v);
}
void launch_block_set_col(hipStream_t s, int n, const double* v, const int* fixed_slot, double* B, int ld, int j) {
  hipLaunchKernelGGL(block_set_col_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, v, fixed_slot, B, ld, j);
}

// X[dof][j] = splitmix64(dof, j, seed) mapped to [-1, 1), zero on pinned rows (tests/modal_np.py hash_block)
__global__ void block_hash_kernel(int n, int m, unsigned seed, const int* __restrict__ fixed_slot, double* __restrict__ B,
                                  int ld) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * m) return;
  const unsigned long long dof = t / m, j = t % m;
  unsigned long long z = dof * 0x9E3779B97F4A7C15ull + j * 0xD1B54A32D192ED03ull +
                         (unsigned long long)seed * 0x94D049BB133111EBull + 0x2545F4914F6CDD1Dull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const bool pinned = fixed_slot && fixed_slot[dof / 3] >= 0;
  B[dof * ld + j] = pinned ? 0.0 : (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}
void launch_block_hash(hipStream_t s, int n, int m, unsigned seed, const int* fixed_slot, double* B, int ld) {
  const size_t tot = (size_t)n * m;
  hipLaunchKernelGGL(block_hash_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, n, m, seed, fixed_slot, B, ld);
}

}  // namespace tlfea
