// contact_kernels.hip -- hydroelastic contact between tetrahedral meshes on gfx950: element-box broadphase on a
// uniform grid, the plane-clipping narrowphase (one work item per pair) and an atomic-free nodal force sum.
//
// Determinism: integer atomics only count or claim slots; every double is written by exactly one thread, and every
// list whose order reaches a double (cell members, pair rows, the contributions of a node) is sorted before use.  The
// results are therefore bitwise reproducible run to run, whatever the scheduling.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "contact_internal.h"

namespace tlfea {
namespace {

constexpr int kBlock = 256;
constexpr int kScanThreads = 1024;

inline int blocks(long long n, int b = kBlock) { return (int)((n + b - 1) / b > 0 ? (n + b - 1) / b : 1); }

struct V3 {
  double x, y, z;
};
__device__ inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline double norm(V3 a) { return sqrt(dot(a, a)); }

// ---- broadphase ------------------------------------------------------------------------------------------------------

__global__ void boxes_kernel(ContactMesh m, ContactPos p, double* __restrict__ box) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m.E) return;
  double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  for (int k = 0; k < m.npe; k++) {
    const int n = m.conn[(size_t)k * m.E + e];
    const double c[3] = {p.x[n], p.y[n], p.z[n]};
    for (int d = 0; d < 3; d++) {
      lo[d] = fmin(lo[d], c[d]);
      hi[d] = fmax(hi[d], c[d]);
    }
  }
  for (int d = 0; d < 3; d++) {
    box[(size_t)e * 6 + d] = lo[d];
    box[(size_t)e * 6 + 3 + d] = hi[d];
  }
}

// one workgroup: bounds of all boxes and the largest box extent -> a cell no smaller than any box (so that two
// overlapping boxes have their lower corners in neighbouring cells), doubled until the grid has at most cell_cap cells
__global__ __launch_bounds__(kBlock) void grid_kernel(int E, const double* __restrict__ box, int cell_cap,
                                                      ContactGrid* grid) {
  __shared__ double s_lo[3][kBlock], s_hi[3][kBlock], s_ext[kBlock];
  const int t = threadIdx.x;
  double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX}, ext = 0.0;
  for (int e = t; e < E; e += kBlock) {
    for (int d = 0; d < 3; d++) {
      const double a = box[(size_t)e * 6 + d], b = box[(size_t)e * 6 + 3 + d];
      lo[d] = fmin(lo[d], a);
      hi[d] = fmax(hi[d], b);
      ext = fmax(ext, b - a);
    }
  }
  for (int d = 0; d < 3; d++) {
    s_lo[d][t] = lo[d];
    s_hi[d][t] = hi[d];
  }
  s_ext[t] = ext;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (t < w) {
      for (int d = 0; d < 3; d++) {
        s_lo[d][t] = fmin(s_lo[d][t], s_lo[d][t + w]);
        s_hi[d][t] = fmax(s_hi[d][t], s_hi[d][t + w]);
      }
      s_ext[t] = fmax(s_ext[t], s_ext[t + w]);
    }
    __syncthreads();
  }
  if (t != 0) return;
  ContactGrid g;
  double range[3];
  bool finite = isfinite(s_ext[0]);
  for (int d = 0; d < 3; d++) {
    g.lo[d] = s_lo[d][0];
    range[d] = s_hi[d][0] - s_lo[d][0];
    finite = finite && isfinite(range[d]) && isfinite(g.lo[d]);
  }
  // the 0.1 % margin keeps floor() of neighbouring lower corners at most one cell apart despite rounding
  double cell = s_ext[0] > 0.0 ? 1.001 * s_ext[0] : 1.0;
  if (!finite || E == 0) {  // non-finite positions: one cell, every pair is tested
    for (int d = 0; d < 3; d++) g.lo[d] = 0.0;
    cell = DBL_MAX;
    range[0] = range[1] = range[2] = 0.0;
  }
  for (;;) {
    double cells = 1.0;
    for (int d = 0; d < 3; d++) {
      g.dim[d] = (int)fmin(floor(range[d] / cell), 1e9) + 1;
      cells *= g.dim[d];
    }
    if (cells <= cell_cap) break;
    cell *= 2.0;
  }
  g.inv_cell = 1.0 / cell;
  g.n_cells = g.dim[0] * g.dim[1] * g.dim[2];
  *grid = g;
}

__device__ inline int cell_coord(double v, double lo, double inv, int dim) {
  const double t = floor((v - lo) * inv);
  if (!(t >= 0.0)) return 0;  // below the grid, or not finite (NaN / -inf): first cell, no int conversion of them
  return t >= (double)(dim - 1) ? dim - 1 : (int)t;
}

__global__ void cell_count_kernel(int E, const double* __restrict__ box, const ContactGrid* __restrict__ grid,
                                  int* __restrict__ elem_cell, int* __restrict__ cell_cnt) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const ContactGrid g = *grid;
  int c[3];
  for (int d = 0; d < 3; d++) c[d] = cell_coord(box[(size_t)e * 6 + d], g.lo[d], g.inv_cell, g.dim[d]);
  const int id = (c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0];
  elem_cell[e] = id;
  atomicAdd(&cell_cnt[id], 1);
}

__global__ __launch_bounds__(kScanThreads) void scan_kernel(const int* __restrict__ cnt, int n, int* __restrict__ off) {
  __shared__ int part[kScanThreads];
  const int t = threadIdx.x;
  const int chunk = (n + kScanThreads - 1) / kScanThreads;
  const int b = min(n, t * chunk), e = min(n, b + chunk);
  int s = 0;
  for (int i = b; i < e; i++) s += cnt[i];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = t ? part[t - 1] : 0;
  for (int i = b; i < e; i++) {
    off[i] = run;
    run += cnt[i];
  }
  if (t == kScanThreads - 1) off[n] = part[kScanThreads - 1];
}

__global__ void cell_fill_kernel(int E, const int* __restrict__ elem_cell, const int* __restrict__ cell_off,
                                 int* __restrict__ cell_cur, int* __restrict__ cell_items) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int c = elem_cell[e];
  cell_items[cell_off[c] + atomicAdd(&cell_cur[c], 1)] = e;
}

__device__ inline bool boxes_overlap(const double* __restrict__ box, int i, int j) {
  for (int d = 0; d < 3; d++) {
    if (box[(size_t)i * 6 + d] > box[(size_t)j * 6 + 3 + d] || box[(size_t)j * 6 + d] > box[(size_t)i * 6 + 3 + d])
      return false;
  }
  return true;
}

__device__ inline bool share_node(const ContactMesh& m, int i, int j) {
  for (int a = 0; a < m.npe; a++) {
    const int n = m.conn[(size_t)a * m.E + i];
    for (int b = 0; b < m.npe; b++)
      if (m.conn[(size_t)b * m.E + j] == n) return true;
  }
  return false;
}

template <bool kFill>
__global__ void pairs_kernel(ContactMesh m, const double* __restrict__ box, const ContactGrid* __restrict__ grid,
                             const int* __restrict__ elem_cell, const int* __restrict__ cell_off,
                             const int* __restrict__ cell_items, int* __restrict__ row_cnt,
                             const int* __restrict__ row_off, int2* __restrict__ pairs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m.E) return;
  const ContactGrid g = *grid;
  const int ci = elem_cell[i];
  const int cx = ci % g.dim[0], cy = (ci / g.dim[0]) % g.dim[1], cz = ci / (g.dim[0] * g.dim[1]);
  const int mi = m.mesh[i];
  const int base = kFill ? row_off[i] : 0;
  int cnt = 0;
  for (int z = max(cz - 1, 0); z <= min(cz + 1, g.dim[2] - 1); z++)
    for (int y = max(cy - 1, 0); y <= min(cy + 1, g.dim[1] - 1); y++)
      for (int x = max(cx - 1, 0); x <= min(cx + 1, g.dim[0] - 1); x++) {
        const int c = (z * g.dim[1] + y) * g.dim[0] + x;
        for (int k = cell_off[c]; k < cell_off[c + 1]; k++) {
          const int j = cell_items[k];
          if (j <= i || !boxes_overlap(box, i, j)) continue;
          if (m.mesh[j] == mi && (!m.self_collision || share_node(m, i, j))) continue;
          if (kFill) pairs[base + cnt] = make_int2(i, j);
          cnt++;
        }
      }
  if (!kFill) {
    row_cnt[i] = cnt;
    return;
  }
  for (int a = base + 1; a < base + cnt; a++) {  // the row in ascending j: the canonical (i, j) order
    const int2 v = pairs[a];
    int b = a - 1;
    while (b >= base && pairs[b].y > v.y) {
      pairs[b + 1] = pairs[b];
      b--;
    }
    pairs[b + 1] = v;
  }
}

// ---- narrowphase -----------------------------------------------------------------------------------------------------

// p(x) = a.x + b through the 4 corner values; false for a degenerate tet
__device__ inline bool affine_fit(const V3 v[4], const double p[4], V3& a, double& b) {
  const V3 e1 = v[1] - v[0], e2 = v[2] - v[0], e3 = v[3] - v[0];
  const V3 c23 = cross(e2, e3), c31 = cross(e3, e1), c12 = cross(e1, e2);
  const double det = dot(e1, c23);
  if (!(fabs(det) > 1e-14 * norm(e1) * norm(e2) * norm(e3))) return false;
  const double inv = 1.0 / det;
  a = inv * ((p[1] - p[0]) * c23 + (p[2] - p[0]) * c31 + (p[3] - p[0]) * c12);
  b = p[0] - dot(a, v[0]);
  return true;
}

// barycentric coordinates of x in the tet v (Cramer's rule)
__device__ inline void barycentric(const V3 v[4], V3 x, double w[4]) {
  const V3 e1 = v[1] - v[0], e2 = v[2] - v[0], e3 = v[3] - v[0], r = x - v[0];
  const double inv = 1.0 / dot(e1, cross(e2, e3));
  w[1] = dot(r, cross(e2, e3)) * inv;
  w[2] = dot(e1, cross(r, e3)) * inv;
  w[3] = dot(e1, cross(e2, r)) * inv;
  w[0] = 1.0 - w[1] - w[2] - w[3];
}

__device__ inline V3 edge_point(V3 a, V3 b, double da, double db) { return a + (da / (da - db)) * (b - a); }

// plane n.x + c = 0 cut with the tet: a triangle (one vertex apart) or a quad (two and two), in cyclic order
__device__ inline int plane_tet(const V3 v[4], V3 n, double c, V3 out[4]) {
  double d[4];
  int pos[4], neg[4], np = 0, nn = 0;
  for (int k = 0; k < 4; k++) {
    d[k] = dot(n, v[k]) + c;
    if (d[k] >= 0.0) pos[np++] = k;
    else neg[nn++] = k;
  }
  if (np == 0 || nn == 0) return 0;
  if (np == 2) {
    const int a = pos[0], b = pos[1], p = neg[0], q = neg[1];
    out[0] = edge_point(v[a], v[p], d[a], d[p]);
    out[1] = edge_point(v[a], v[q], d[a], d[q]);
    out[2] = edge_point(v[b], v[q], d[b], d[q]);
    out[3] = edge_point(v[b], v[p], d[b], d[p]);
    return 4;
  }
  const int* one = np == 1 ? pos : neg;
  const int* three = np == 1 ? neg : pos;
  for (int k = 0; k < 3; k++) out[k] = edge_point(v[one[0]], v[three[k]], d[one[0]], d[three[k]]);
  return 3;
}

// Sutherland-Hodgman: keep the part of the polygon inside the tet (4 half-spaces; at most 8 vertices)
__device__ inline int clip_tet(V3 poly[8], int cnt, const V3 v[4]) {
  V3 tmp[8];
  for (int f = 0; f < 4 && cnt > 0; f++) {
    const V3 q0 = v[(f + 1) & 3], q1 = v[(f + 2) & 3], q2 = v[(f + 3) & 3];
    V3 nf = cross(q1 - q0, q2 - q0);
    if (dot(nf, v[f] - q0) < 0.0) nf = -1.0 * nf;  // inward: towards the vertex opposite the face
    int m = 0;
    for (int k = 0; k < cnt; k++) {
      const V3 P = poly[k], Q = poly[(k + 1) % cnt];
      const double sp = dot(nf, P - q0), sq = dot(nf, Q - q0);
      if (sp >= 0.0 && m < 8) tmp[m++] = P;
      if ((sp >= 0.0) != (sq >= 0.0) && m < 8) tmp[m++] = edge_point(P, Q, sp, sq);
    }
    cnt = m;
    for (int k = 0; k < cnt; k++) poly[k] = tmp[k];
  }
  return cnt;
}

__device__ inline void corners(const ContactMesh& m, ContactPos p, int e, V3 v[4], double pr[4]) {
  for (int k = 0; k < 4; k++) {
    const int n = m.conn[(size_t)k * m.E + e];
    v[k] = {p.x[n], p.y[n], p.z[n]};
    if (pr) pr[k] = m.press[n];
  }
}

__global__ void narrowphase_kernel(ContactMesh m, ContactPos p, int n_pairs, const int2* __restrict__ pairs,
                                   tlfea_contact_patch* __restrict__ patches, int* __restrict__ n_valid) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_pairs) return;
  int A = pairs[k].x, B = pairs[k].y;
  if (m.mesh[A] > m.mesh[B]) {  // tet A on the lower mesh id: the normal points from the lower id to the higher one
    const int t = A;
    A = B;
    B = t;
  }
  V3 poly[8] = {};
  int cnt = 0;
  V3 nhat = {0, 0, 0}, cen = {0, 0, 0};
  double area = 0.0, gA = 0.0, gB = 0.0, peq = 0.0;
  bool valid = false, orient = false;
  V3 vA[4], vB[4], aA, aB;
  double pA[4], pB[4], bA, bB;
  corners(m, p, A, vA, pA);
  corners(m, p, B, vB, pB);
  if (affine_fit(vA, pA, aA, bA) && affine_fit(vB, pB, aB, bB)) {
    const V3 n = aA - aB;
    const double c = bA - bB, nn = norm(n);
    if (nn >= 1e-9) {
      cnt = plane_tet(vA, n, c, poly);
      if (cnt >= 3) cnt = clip_tet(poly, cnt, vB);
      if (cnt >= 3) {
        V3 s = {0, 0, 0};
        for (int i = 1; i + 1 < cnt; i++) s = s + cross(poly[i] - poly[0], poly[i + 1] - poly[0]);
        const double sn = norm(s);
        area = 0.5 * sn;
        if (area >= 1e-18) {
          const V3 u = (1.0 / sn) * s;
          double wsum = 0.0;
          V3 acc = {0, 0, 0};
          for (int i = 1; i + 1 < cnt; i++) {
            const double w = dot(cross(poly[i] - poly[0], poly[i + 1] - poly[0]), u);
            acc = acc + w * (poly[0] + poly[i] + poly[i + 1]);
            wsum += w;
          }
          cen = (1.0 / (3.0 * wsum)) * acc;
          nhat = (1.0 / nn) * n;
          gA = -dot(aA, nhat);
          gB = dot(aB, nhat);
          orient = true;
          if (gA <= 0.0 || gB <= 0.0) {
            nhat = -1.0 * nhat;
            gA = -gA;
            gB = -gB;
            if (gA <= 0.0 || gB <= 0.0) {  // no consistent direction: keep the plane normal, apply nothing
              orient = false;
              nhat = -1.0 * nhat;
              gA = -gA;
              gB = -gB;
            }
          }
          peq = dot(aA, cen) + bA;
          valid = true;
        }
      }
    }
  }
  if (!valid) {
    cnt = 0;
    area = 0.0;
  }
  tlfea_contact_patch& P = patches[k];
  for (int i = 0; i < 8; i++) {
    const V3 q = i < cnt ? poly[i] : V3{0, 0, 0};
    P.vertices[i][0] = q.x;
    P.vertices[i][1] = q.y;
    P.vertices[i][2] = q.z;
  }
  P.count = cnt;
  P.normal[0] = nhat.x, P.normal[1] = nhat.y, P.normal[2] = nhat.z;
  P.centroid[0] = cen.x, P.centroid[1] = cen.y, P.centroid[2] = cen.z;
  P.area = area;
  P.g_A = gA;
  P.g_B = gB;
  P.p_equilibrium = peq;
  P.tetA = A;
  P.tetB = B;
  P.isValid = valid;
  P.validOrientation = valid && orient;
  if (valid) atomicAdd(n_valid, 1);
}

// ---- forces ----------------------------------------------------------------------------------------------------------

__global__ void forces_kernel(ContactMesh m, ContactPos p, int n_pairs, const tlfea_contact_patch* __restrict__ patches,
                              const double* __restrict__ vel, double damping, double friction,
                              double* __restrict__ contrib, int* __restrict__ slot_node, int* __restrict__ node_cnt) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_pairs) return;
  const tlfea_contact_patch& P = patches[k];
  const bool act = P.isValid && P.validOrientation && P.area > 1e-18;
  int node[8];
  const int A = P.tetA, B = P.tetB;
  for (int i = 0; i < 4; i++) {
    node[i] = m.conn[(size_t)i * m.E + A];
    node[4 + i] = m.conn[(size_t)i * m.E + B];
  }
  if (!act) {
    for (int s = 0; s < 8; s++) slot_node[(size_t)k * 8 + s] = -1;
    return;
  }
  V3 vA[4], vB[4];
  corners(m, p, A, vA, nullptr);
  corners(m, p, B, vB, nullptr);
  const V3 n = {P.normal[0], P.normal[1], P.normal[2]}, cen = {P.centroid[0], P.centroid[1], P.centroid[2]};
  double wA[4], wB[4];
  barycentric(vA, cen, wA);
  barycentric(vB, cen, wB);
  double pd = P.p_equilibrium;
  const bool rel = vel != nullptr && (damping > 0.0 || friction > 0.0);
  V3 vr = {0, 0, 0};
  double vn = 0.0;
  if (rel) {
    for (int i = 0; i < 4; i++) {
      const V3 va = {vel[3 * node[i]], vel[3 * node[i] + 1], vel[3 * node[i] + 2]};
      const V3 vb = {vel[3 * node[4 + i]], vel[3 * node[4 + i] + 1], vel[3 * node[4 + i] + 2]};
      vr = vr + (wB[i] * vb - wA[i] * va);
    }
    vn = dot(vr, n);
    if (damping > 0.0) pd = pd * fmax(0.0, 1.0 - damping * vn);
  }
  V3 F = (pd * P.area) * n;
  if (rel && friction > 0.0) {
    const V3 vt = vr - vn * n;
    const double st = norm(vt);
    if (st > 0.0) F = F - (friction * fabs(pd * P.area) * (st / (st + 1e-3)) / st) * vt;
  }
  for (int s = 0; s < 8; s++) {
    const double w = s < 4 ? -wA[s] : wB[s - 4];
    contrib[((size_t)k * 8 + s) * 3 + 0] = w * F.x;
    contrib[((size_t)k * 8 + s) * 3 + 1] = w * F.y;
    contrib[((size_t)k * 8 + s) * 3 + 2] = w * F.z;
    slot_node[(size_t)k * 8 + s] = node[s];
    atomicAdd(&node_cnt[node[s]], 1);
  }
}

__global__ void node_fill_kernel(int n_slots, const int* __restrict__ slot_node, const int* __restrict__ node_off,
                                 int* __restrict__ node_cur, int* __restrict__ node_items) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_slots) return;
  const int n = slot_node[k];
  if (n < 0) return;
  node_items[node_off[n] + atomicAdd(&node_cur[n], 1)] = k;
}

__global__ void node_sum_kernel(int N, const int* __restrict__ node_off, int* __restrict__ node_items,
                                const double* __restrict__ contrib, double* __restrict__ force) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int b = node_off[n], e = node_off[n + 1];
  for (int i = b + 1; i < e; i++) {  // ascending (patch, slot): the summation order does not depend on scheduling
    const int v = node_items[i];
    int j = i - 1;
    while (j >= b && node_items[j] > v) {
      node_items[j + 1] = node_items[j];
      j--;
    }
    node_items[j + 1] = v;
  }
  double f[3] = {0.0, 0.0, 0.0};
  for (int i = b; i < e; i++) {
    const size_t s = (size_t)node_items[i] * 3;
    f[0] += contrib[s];
    f[1] += contrib[s + 1];
    f[2] += contrib[s + 2];
  }
  force[3 * (size_t)n] = f[0];
  force[3 * (size_t)n + 1] = f[1];
  force[3 * (size_t)n + 2] = f[2];
}

__global__ void add_kernel(int n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

}  // namespace

void launch_contact_boxes(hipStream_t s, const ContactMesh& m, ContactPos p, double* box) {
  hipLaunchKernelGGL(boxes_kernel, dim3(blocks(m.E)), dim3(kBlock), 0, s, m, p, box);
}
void launch_contact_grid(hipStream_t s, int E, const double* box, int cell_cap, ContactGrid* grid) {
  hipLaunchKernelGGL(grid_kernel, dim3(1), dim3(kBlock), 0, s, E, box, cell_cap, grid);
}
void launch_contact_cell_count(hipStream_t s, int E, const double* box, const ContactGrid* grid, int* elem_cell,
                               int* cell_cnt) {
  hipLaunchKernelGGL(cell_count_kernel, dim3(blocks(E)), dim3(kBlock), 0, s, E, box, grid, elem_cell, cell_cnt);
}
void launch_contact_scan(hipStream_t s, const int* cnt, int n, int* off) {
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScanThreads), 0, s, cnt, n, off);
}
void launch_contact_cell_fill(hipStream_t s, int E, const int* elem_cell, const int* cell_off, int* cell_cur,
                              int* cell_items) {
  hipLaunchKernelGGL(cell_fill_kernel, dim3(blocks(E)), dim3(kBlock), 0, s, E, elem_cell, cell_off, cell_cur,
                     cell_items);
}
void launch_contact_pairs(hipStream_t s, const ContactMesh& m, const double* box, const ContactGrid* grid,
                          const int* elem_cell, const int* cell_off, const int* cell_items, bool fill, int* row_cnt,
                          const int* row_off, int2* pairs) {
  if (fill)
    hipLaunchKernelGGL(pairs_kernel<true>, dim3(blocks(m.E)), dim3(kBlock), 0, s, m, box, grid, elem_cell, cell_off,
                       cell_items, row_cnt, row_off, pairs);
  else
    hipLaunchKernelGGL(pairs_kernel<false>, dim3(blocks(m.E)), dim3(kBlock), 0, s, m, box, grid, elem_cell, cell_off,
                       cell_items, row_cnt, row_off, pairs);
}
void launch_contact_narrowphase(hipStream_t s, const ContactMesh& m, ContactPos p, int n_pairs, const int2* pairs,
                                tlfea_contact_patch* patches, int* n_valid) {
  hipLaunchKernelGGL(narrowphase_kernel, dim3(blocks(n_pairs)), dim3(kBlock), 0, s, m, p, n_pairs, pairs, patches,
                     n_valid);
}
void launch_contact_forces(hipStream_t s, const ContactMesh& m, ContactPos p, int n_pairs,
                           const tlfea_contact_patch* patches, const double* vel, double damping, double friction,
                           double* contrib, int* slot_node, int* node_cnt) {
  hipLaunchKernelGGL(forces_kernel, dim3(blocks(n_pairs)), dim3(kBlock), 0, s, m, p, n_pairs, patches, vel, damping,
                     friction, contrib, slot_node, node_cnt);
}
void launch_contact_node_fill(hipStream_t s, int n_slots, const int* slot_node, const int* node_off, int* node_cur,
                              int* node_items) {
  hipLaunchKernelGGL(node_fill_kernel, dim3(blocks(n_slots)), dim3(kBlock), 0, s, n_slots, slot_node, node_off,
                     node_cur, node_items);
}
void launch_contact_node_sum(hipStream_t s, int N, const int* node_off, int* node_items, const double* contrib,
                             double* force) {
  hipLaunchKernelGGL(node_sum_kernel, dim3(blocks(N)), dim3(kBlock), 0, s, N, node_off, node_items, contrib, force);
}
void launch_contact_add(hipStream_t s, int n, const double* a, const double* b, double* out) {
  hipLaunchKernelGGL(add_kernel, dim3(blocks(n)), dim3(kBlock), 0, s, n, a, b, out);
}

}  // namespace tlfea
