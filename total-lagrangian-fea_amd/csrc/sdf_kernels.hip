// sdf_kernels.hip -- signed distance of a closed triangle surface on a regular grid (tlfea_sdf_from_triangles,
// DESIGN 3e''): the builder of the field obstacles.
//
//   sdf_from_triangles_kernel  one thread per grid sample; the triangles (9 doubles each) pass through LDS in tiles of
//                              kSdfTile and every thread walks them in ascending order, keeping the smallest squared
//                              point-triangle distance (closest point by Voronoi region, Ericson) and the sum of the
//                              signed solid angles (van Oosterom-Strackee).  Value: -d where |sum| / 4 pi >= 1/2, else +d.
//
// fp64 throughout, a fixed order and no atomics: the grid is bitwise reproducible.  The sign is the winding number's, so
// it needs no pseudo-normals and holds for an inward as for an outward orientation, as long as it is consistent.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tlfea_internal.h"

namespace tlfea {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// squared distance from the origin to the triangle (a, b, c): vertices relative to the query point
__device__ __forceinline__ double tri_dist2(const double a[3], const double b[3], const double c[3]) {
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double d1 = -dot3(ab, a), d2 = -dot3(ac, a);  // ap = -a
  if (d1 <= 0.0 && d2 <= 0.0) return dot3(a, a);      // vertex a
  const double d3 = -dot3(ab, b), d4 = -dot3(ac, b);
  if (d3 >= 0.0 && d4 <= d3) return dot3(b, b);       // vertex b
  const double vc = d1 * d4 - d3 * d2;
  double v, w;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {          // edge ab
    v = d1 / (d1 - d3);
    w = 0.0;
  } else {
    const double d5 = -dot3(ab, c), d6 = -dot3(ac, c);
    if (d6 >= 0.0 && d5 <= d6) return dot3(c, c);     // vertex c
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {        // edge ac
      v = 0.0;
      w = d2 / (d2 - d6);
    } else {
      const double va = d3 * d6 - d5 * d4;
      if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {  // edge bc
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        v = 1.0 - w;
      } else {                                        // interior
        const double den = 1.0 / (va + vb + vc);
        v = vb * den;
        w = vc * den;
      }
    }
  }
  const double r[3] = {a[0] + v * ab[0] + w * ac[0], a[1] + v * ab[1] + w * ac[1], a[2] + v * ab[2] + w * ac[2]};
  return dot3(r, r);
}

// signed solid angle of the triangle (a, b, c) seen from the origin
__device__ __forceinline__ double tri_solid_angle(const double a[3], const double b[3], const double c[3]) {
  const double la = sqrt(dot3(a, a)), lb = sqrt(dot3(b, b)), lc = sqrt(dot3(c, c));
  const double det = a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) +
                     a[2] * (b[0] * c[1] - b[1] * c[0]);
  const double den = la * lb * lc + dot3(a, b) * lc + dot3(b, c) * la + dot3(c, a) * lb;
  return 2.0 * atan2(det, den);
}

__global__ __launch_bounds__(kBlock) void sdf_from_triangles_kernel(const double* __restrict__ tri, int n_tris, int nx,
                                                                    int ny, double ox, double oy, double oz,
                                                                    double spacing, long long first, long long count,
                                                                    double* __restrict__ out) {
  __shared__ double T[kSdfTile * 9];
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = k < count;
  const long long s = first + (live ? k : 0);  // an idle thread walks sample `first`: it takes part in the barriers
  const int ix = (int)(s % nx), iy = (int)((s / nx) % ny), iz = (int)(s / ((long long)nx * ny));
  const double p[3] = {ox + spacing * ix, oy + spacing * iy, oz + spacing * iz};
  double d2 = INFINITY, omega = 0.0;
  for (int t0 = 0; t0 < n_tris; t0 += kSdfTile) {
    const int nt = n_tris - t0 < kSdfTile ? n_tris - t0 : kSdfTile;
    __syncthreads();
    for (int i = threadIdx.x; i < nt * 9; i += kBlock) T[i] = tri[(size_t)t0 * 9 + i];
    __syncthreads();
    for (int t = 0; t < nt; t++) {
      const double* v = T + 9 * t;
      const double a[3] = {v[0] - p[0], v[1] - p[1], v[2] - p[2]};
      const double b[3] = {v[3] - p[0], v[4] - p[1], v[5] - p[2]};
      const double c[3] = {v[6] - p[0], v[7] - p[1], v[8] - p[2]};
      const double e = tri_dist2(a, b, c);
      d2 = e < d2 ? e : d2;
      omega += tri_solid_angle(a, b, c);
    }
  }
  if (!live) return;
  const double d = sqrt(d2);
  out[s] = fabs(omega) / (4.0 * M_PI) >= 0.5 ? -d : d;
}

}  // namespace

void launch_sdf_from_triangles(hipStream_t s, const double* tri, int n_tris, int nx, int ny, const double origin[3],
                               double spacing, long long first, long long count, double* out) {
  if (count <= 0) return;
  const long long blocks = (count + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(sdf_from_triangles_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, tri, n_tris, nx, ny, origin[0],
                     origin[1], origin[2], spacing, first, count, out);
}

}  // namespace tlfea
