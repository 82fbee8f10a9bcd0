// Test shim: exposes the lists of the streamed build of the restricted fine operator (csrc/pmg_host.h: con_pos by source,
// the prefix per child, the rows beyond the image's capacity) to ctypes, so that the CPU suite can check them without a
// GPU.  Built by tests/test_rop_stream_host.py with g++.
#include "../../total-lagrangian-fea_amd/csrc/pmg_host.h"

static tlfea::PmgHost g_h;
static tlfea::RopHost g_r;

// conn: column-major [10][E]; off/cols: fine node adjacency (sorted).  sizes: Nc, blocks of R, contributions, children
extern "C" int rops_build(int N, int E, const int* conn, const int* off, const int* cols, int* sizes) {
  if (!tlfea::pmg_build(N, E, conn, off, cols, g_h)) return 1;
  if (!tlfea::pmg_restrict_op_build(N, off, cols, g_h, g_r)) return 2;
  sizes[0] = g_r.Nc;
  sizes[1] = g_r.nnz;
  sizes[2] = g_r.n_con;
  sizes[3] = (int)g_r.ch.size();
  return 0;
}
extern "C" void rops_fetch(int* par0, int* par1, int* r_off, int* r_cols, int* ch_off, int* ch, float* ch_w, int* pos_off,
                           unsigned short* con_pos) {
  std::copy(g_h.par0.begin(), g_h.par0.end(), par0);
  std::copy(g_h.par1.begin(), g_h.par1.end(), par1);
  std::copy(g_r.off.begin(), g_r.off.end(), r_off);
  std::copy(g_r.cols.begin(), g_r.cols.end(), r_cols);
  std::copy(g_r.ch_off.begin(), g_r.ch_off.end(), ch_off);
  std::copy(g_r.ch.begin(), g_r.ch.end(), ch);
  std::copy(g_r.ch_w.begin(), g_r.ch_w.end(), ch_w);
  std::copy(g_r.pos_off.begin(), g_r.pos_off.end(), pos_off);
  std::copy(g_r.con_pos.begin(), g_r.con_pos.end(), con_pos);
}
// rows longer than cap blocks into rows [Nc]; returns their number
extern "C" int rops_long_rows(int cap, int* rows) {
  const std::vector<int> v = tlfea::pmg_rop_long_rows(g_r, cap);
  std::copy(v.begin(), v.end(), rows);
  return (int)v.size();
}
