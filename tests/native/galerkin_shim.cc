// Test shim: exposes the host set-up of the vertex-level Galerkin gather (csrc/pmg_host.h: the contribution lists of the
// blocks with column >= row, c_upper and c_mirror; integer work only) to ctypes, so that the CPU suite can execute the
// lists in NumPy without a GPU.  Built by tests/test_galerkin_host.py with g++.
#include "../../total-lagrangian-fea_amd/csrc/pmg_host.h"

static tlfea::PmgHost g_h;

static void sizes_of(int* sizes) {
  sizes[0] = g_h.Nc;
  sizes[1] = g_h.nnz_c;
  sizes[2] = (int)g_h.c_upper.size();
  sizes[3] = (int)g_h.con_w.size();
}
// conn: column-major [10][E]; off/cols: fine node adjacency (sorted).  sizes: Nc, coarse blocks, upper blocks, contributions
extern "C" int gal_build(int N, int E, const int* conn, const int* off, const int* cols, int* sizes) {
  if (!tlfea::pmg_build(N, E, conn, off, cols, g_h)) return 1;
  sizes_of(sizes);
  return 0;
}
// the ANCF builder: N coefficients (four per node), their adjacency
extern "C" int gal_build_ancf(int N, const int* off, const int* cols, int* sizes) {
  if (!tlfea::pmg_build_ancf(N, off, cols, g_h)) return 1;
  sizes_of(sizes);
  return 0;
}
extern "C" void gal_fetch(int* par0, int* par1, int* c_off, int* c_cols, int* cblk_row, int* c_upper, int* c_mirror,
                          int* con_off, int* con_blk, int* con_base, int* con_deg, float* con_w) {
  std::copy(g_h.par0.begin(), g_h.par0.end(), par0);
  std::copy(g_h.par1.begin(), g_h.par1.end(), par1);
  std::copy(g_h.c_off.begin(), g_h.c_off.end(), c_off);
  std::copy(g_h.c_cols.begin(), g_h.c_cols.end(), c_cols);
  std::copy(g_h.cblk_row.begin(), g_h.cblk_row.end(), cblk_row);
  std::copy(g_h.c_upper.begin(), g_h.c_upper.end(), c_upper);
  std::copy(g_h.c_mirror.begin(), g_h.c_mirror.end(), c_mirror);
  std::copy(g_h.con_off.begin(), g_h.con_off.end(), con_off);
  std::copy(g_h.con_blk.begin(), g_h.con_blk.end(), con_blk);
  std::copy(g_h.con_base.begin(), g_h.con_base.end(), con_base);
  std::copy(g_h.con_deg.begin(), g_h.con_deg.end(), con_deg);
  std::copy(g_h.con_w.begin(), g_h.con_w.end(), con_w);
}
// the mirror table of the last build's coarse pattern with block `drop` taken out: 1 = accepted, 0 = refused
extern "C" int gal_mirror_without(int drop) {
  tlfea::PmgHost h;
  h.Nc = g_h.Nc;
  h.c_off.assign((size_t)h.Nc + 1, 0);
  for (int cb = 0; cb < g_h.nnz_c; cb++) {
    if (cb == drop) continue;
    h.c_cols.push_back(g_h.c_cols[cb]);
    h.cblk_row.push_back(g_h.cblk_row[cb]);
    h.c_off[(size_t)g_h.cblk_row[cb] + 1]++;
  }
  for (int I = 0; I < h.Nc; I++) h.c_off[I + 1] += h.c_off[I];
  h.nnz_c = (int)h.c_cols.size();
  std::vector<int> upos;
  return tlfea::pmg_mirror_build(h, upos) ? 1 : 0;
}
