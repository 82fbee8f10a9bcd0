// C entry points of csrc/matfree_compact.h for tests/test_matfree_compact_host.py (the header is pure host code).
#include "../../total-lagrangian-fea_amd/csrc/matfree_compact.h"

#include <cstring>

static tlfea::MatfreeCompactHost g_mc;
static int g_E = 0;

// conn: column-major [10][E].  sizes4 = {wavefronts, rows, largest number of rows of one node, slots per wavefront}
extern "C" int mfc_build(int N, int E, const int* conn, int* sizes4) {
  if (!tlfea::build_matfree_compact(N, E, conn, g_mc)) return 1;
  g_E = E;
  sizes4[0] = g_mc.W;
  sizes4[1] = (int)g_mc.rows();
  sizes4[2] = g_mc.max_rows_per_node;
  sizes4[3] = tlfea::kMfcSrc;
  return 0;
}
extern "C" double mfc_ratio() { return g_mc.ratio(g_E); }
// row_off [W + 1], row_node [rows], desc [W * 640], src [W * 640], n2r_off [N + 1], n2r [rows]
extern "C" void mfc_copy(int* row_off, int* row_node, unsigned short* desc, unsigned short* src, int* n2r_off, int* n2r) {
  std::memcpy(row_off, g_mc.row_off.data(), g_mc.row_off.size() * sizeof(int));
  std::memcpy(row_node, g_mc.row_node.data(), g_mc.row_node.size() * sizeof(int));
  std::memcpy(desc, g_mc.desc.data(), g_mc.desc.size() * sizeof(unsigned short));
  std::memcpy(src, g_mc.src.data(), g_mc.src.size() * sizeof(unsigned short));
  std::memcpy(n2r_off, g_mc.n2r_off.data(), g_mc.n2r_off.size() * sizeof(int));
  std::memcpy(n2r, g_mc.n2r.data(), g_mc.n2r.size() * sizeof(int));
}
