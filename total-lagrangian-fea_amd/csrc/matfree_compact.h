// matfree_compact.h -- per-wavefront compaction of the element rows of the matrix-free product q = H p.
//
// Pure host code: no HIP, no environment, no state.  Built once per mesh from the connectivity.
//
// tangent_apply_affine_kernel gives wavefront w the elements [64 w, min(E, 64 w + 64)), one per lane, and every element
// produces one 24-byte row per local node.  Neighbouring elements share nodes, so most of a wavefront's 640 rows are
// partial sums of the same node.  The kernel adds them up before they leave the CU:
//   compact rows   the wavefront's unique global nodes in ascending order; row_off[w] is the prefix sum over wavefronts,
//                  row_off[W] the length of the row buffer [rows][3]
//   desc           start | (count - 1) << 10 of row s of wavefront w at desc[640 w + s]: the row's sources are
//                  src[640 w + start .. + count).  A fixed 640 slots per wavefront (a wavefront has at most 640 rows)
//                  keeps its slice 4-byte aligned for the kernel's staging loads; only the first rows(w) slots are read.
//   src            16-bit LDS row indices a * 64 + lane of the (element, local node) pairs that hit the row's node, in
//                  ascending element (= lane) order; a node occurs at most once per element, so count <= 64.  Lanes past
//                  E are padding and are a source of nothing.  640 entries per wavefront, the unused tail is 0.
//   n2r_off, n2r   node -> its compact rows, ascending (rows are numbered wavefront by wavefront, so ascending wavefront)
// Summation order of q_i, fixed: ascending element inside a wavefront, then ascending wavefront.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace tlfea {

constexpr int kMfcWave = 64;                    // elements per wavefront
constexpr int kMfcNodes = 10;                   // local nodes of a T10 element
constexpr int kMfcSrc = kMfcWave * kMfcNodes;   // LDS rows (and source entries) per wavefront
constexpr int kMfcStartBits = 10;               // desc: start in the low 10 bits (< 640), count - 1 above (< 64)

struct MatfreeCompactHost {
  int W = 0;                      // wavefronts
  std::vector<int> row_off;       // [W + 1]
  std::vector<int> row_node;      // [rows] global node of a compact row (host only: tests, n2r)
  std::vector<uint16_t> desc;     // [W * 640]
  std::vector<uint16_t> src;      // [W * 640]
  std::vector<int> n2r_off, n2r;  // [N + 1], [rows]
  int max_rows_per_node = 0;
  long rows() const { return row_off.empty() ? 0 : row_off.back(); }
  double ratio(int E) const { return rows() > 0 ? (double)kMfcNodes * E / (double)rows() : 0.0; }  // 10 E / rows
};

// conn: column-major [10][E] global nodes.  False on a malformed mesh (node out of range, a node twice in one element).
inline bool build_matfree_compact(int N, int E, const int* conn, MatfreeCompactHost& out) {
  if (N <= 0 || E <= 0) return false;
  const int W = (E + kMfcWave - 1) / kMfcWave;
  out.W = W;
  out.row_off.assign((size_t)W + 1, 0);
  out.row_node.clear();
  out.desc.assign((size_t)W * kMfcSrc, 0);
  out.src.assign((size_t)W * kMfcSrc, 0);
  out.row_node.reserve((size_t)E * 4);
  std::vector<std::pair<int, int>> key;  // (node, lane * 16 + a): sorts by node, then element, then local node
  key.reserve(kMfcSrc);
  for (int w = 0; w < W; w++) {
    const int e0 = w * kMfcWave, n_el = std::min(kMfcWave, E - e0);
    key.clear();
    for (int l = 0; l < n_el; l++)
      for (int a = 0; a < kMfcNodes; a++) {
        const int node = conn[(size_t)a * E + e0 + l];
        if (node < 0 || node >= N) return false;
        key.emplace_back(node, l * 16 + a);
      }
    std::sort(key.begin(), key.end());
    uint16_t* src = out.src.data() + (size_t)w * kMfcSrc;
    uint16_t* desc = out.desc.data() + (size_t)w * kMfcSrc - out.row_off[w];
    for (size_t k = 0; k < key.size();) {
      size_t k1 = k;
      while (k1 < key.size() && key[k1].first == key[k].first) {
        if (k1 > k && (key[k1].second >> 4) == (key[k1 - 1].second >> 4)) return false;  // twice in one element
        src[k1] = (uint16_t)((key[k1].second & 15) * kMfcWave + (key[k1].second >> 4));
        k1++;
      }
      desc[out.row_node.size()] = (uint16_t)(k | ((k1 - k - 1) << kMfcStartBits));
      out.row_node.push_back(key[k].first);
      k = k1;
    }
    out.row_off[w + 1] = (int)out.row_node.size();
  }
  const int rows = (int)out.row_node.size();
  out.n2r_off.assign((size_t)N + 1, 0);
  for (int r = 0; r < rows; r++) out.n2r_off[out.row_node[r] + 1]++;
  out.max_rows_per_node = 0;
  for (int i = 0; i < N; i++) {
    out.max_rows_per_node = std::max(out.max_rows_per_node, out.n2r_off[i + 1]);
    out.n2r_off[i + 1] += out.n2r_off[i];
  }
  out.n2r.assign((size_t)rows, 0);
  std::vector<int> cur(out.n2r_off.begin(), out.n2r_off.end() - 1);
  for (int r = 0; r < rows; r++) out.n2r[cur[out.row_node[r]]++] = r;  // ascending r per node
  return true;
}

}  // namespace tlfea
