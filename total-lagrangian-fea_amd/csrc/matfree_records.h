// matfree_records.h -- packed, lane-major element records of the matrix-free passes (DESIGN 3g, 3g').
//
// Index functions only: no HIP call, no environment, no state.  The apply kernel, the pack kernel and the host tests share
// this one definition.
//
// tangent_apply_affine_kernel gives wavefront w the 64 elements of tile w (the dealing of matfree_compact.h), one per
// lane.  The element-major records ([E][16] of g, [E][5][10] of F) make a lane's values 128 / 400 bytes apart, so the
// kernel had to transpose them through LDS.  Here value t of lane l of a tile lies at [tile][t][l], with consecutive t
// grouped so that one lane's load is 16 bytes (2 doubles, 4 floats); the group at the end of a sub-record is as long as
// what is left (1 or 2 values).  Every wavefront load is then one contiguous run of 64 x (group bytes).
//   g record   10 values per element: g_0, g_1, g_2 (3 each), det J.  g_3 = -(g_0 + g_1 + g_2), since sum_n L_n = 1.
//   F record   NP sub-records of 9 values (F row-major) per element, one per stored point.  NP = 5: the slot order of
//              the residual launch (centroid, then the points of vertices 0..3).  NP = 4: the points of vertices 0..3
//              only -- F is linear over an affine element, so the centroid's F is the mean of the other four.
// The last tile is padded to 64 lanes; the padding lanes hold a copy of the last element.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define TLFEA_MFR_HD __host__ __device__
#else
#define TLFEA_MFR_HD
#endif

namespace tlfea {

constexpr int kMfrWave = 64;      // elements per tile
constexpr int kMfrGVals = 10;     // values of a g record
constexpr int kMfrFVals = 9;      // values of F at one point
constexpr int kMfrLoadBytes = 16; // a lane's widest load

// values per full group for a real type of `real_bytes` bytes
TLFEA_MFR_HD constexpr int mfr_group(int real_bytes) { return kMfrLoadBytes / real_bytes; }
TLFEA_MFR_HD constexpr size_t mfr_tiles(size_t E) { return (E + kMfrWave - 1) / kMfrWave; }
// length of the group that holds value t of a sub-record of T values
TLFEA_MFR_HD constexpr int mfr_group_len(int T, int G, int t) { return T - t / G * G < G ? T - t / G * G : G; }
// offset of value t of lane `lane` inside a tile's sub-record of T values (64 T slots)
TLFEA_MFR_HD constexpr size_t mfr_sub_index(int T, int G, int lane, int t) {
  return (size_t)(t / G * G) * kMfrWave + (size_t)lane * mfr_group_len(T, G, t) + (size_t)(t % G);
}
// g record: value t (0..9) of element e
TLFEA_MFR_HD constexpr size_t mfr_g_index(int G, size_t e, int t) {
  return e / kMfrWave * (kMfrGVals * kMfrWave) + mfr_sub_index(kMfrGVals, G, (int)(e % kMfrWave), t);
}
// F record: value t (0..8) at stored point p (0..NP-1) of element e
TLFEA_MFR_HD constexpr size_t mfr_F_index(int NP, int G, size_t e, int p, int t) {
  return (e / kMfrWave * NP + p) * (size_t)(kMfrFVals * kMfrWave) + mfr_sub_index(kMfrFVals, G, (int)(e % kMfrWave), t);
}
TLFEA_MFR_HD constexpr size_t mfr_g_len(size_t E) { return mfr_tiles(E) * kMfrWave * kMfrGVals; }
TLFEA_MFR_HD constexpr size_t mfr_F_len(size_t E, int NP) { return mfr_tiles(E) * kMfrWave * kMfrFVals * NP; }
// where the values come from: g value t in the [E][16] record (g_n at 4 n .. 4 n + 2, det J at 3), slot of stored point p
// in the [E][5][10] record
TLFEA_MFR_HD constexpr int mfr_g_source(int t) { return t == kMfrGVals - 1 ? 3 : 4 * (t / 3) + t % 3; }
TLFEA_MFR_HD constexpr int mfr_F_slot(int NP, int p) { return NP == 4 ? p + 1 : p; }

}  // namespace tlfea
