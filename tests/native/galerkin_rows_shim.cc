// Test shim: exposes the lists of the Galerkin operator summed from the row image of R (csrc/pmg_host.h: RopHost's row
// structure and GalRowsHost's combine) to ctypes, so that the CPU suite can check them without a GPU.  Built by
// tests/test_galerkin_rows_host.py with g++.
#include "../../total-lagrangian-fea_amd/csrc/pmg_host.h"

static tlfea::PmgHost g_h;
static tlfea::RopHost g_r;
static tlfea::GalRowsHost g_g;

// conn: column-major [10][E]; off/cols: fine node adjacency (sorted).  sizes: Nc, blocks of R, contributions, children,
// coarse blocks, upper coarse blocks, terms of the combine
extern "C" int galr_build(int N, int E, const int* conn, const int* off, const int* cols, int* sizes) {
  if (!tlfea::pmg_build(N, E, conn, off, cols, g_h)) return 1;
  if (!tlfea::pmg_restrict_op_build(N, off, cols, g_h, g_r)) return 2;
  if (!tlfea::pmg_galerkin_rows_build(g_h, g_r, g_g)) return 3;
  sizes[0] = g_r.Nc;
  sizes[1] = g_r.nnz;
  sizes[2] = g_r.n_con;
  sizes[3] = (int)g_r.ch.size();
  sizes[4] = g_h.nnz_c;
  sizes[5] = (int)g_h.c_upper.size();
  sizes[6] = (int)g_g.term_pos.size();
  return 0;
}
extern "C" void galr_fetch_rows(int* par0, int* par1, int* r_off, int* r_cols, int* ch_off, int* ch, float* ch_w, int* pos_off,
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
extern "C" void galr_fetch_combine(int* c_off, int* c_cols, int* cblk_row, int* c_upper, int* c_mirror, int* row_off,
                                   int* term_off, unsigned short* term_pos, unsigned char* term_w) {
  std::copy(g_h.c_off.begin(), g_h.c_off.end(), c_off);
  std::copy(g_h.c_cols.begin(), g_h.c_cols.end(), c_cols);
  std::copy(g_h.cblk_row.begin(), g_h.cblk_row.end(), cblk_row);
  std::copy(g_h.c_upper.begin(), g_h.c_upper.end(), c_upper);
  std::copy(g_h.c_mirror.begin(), g_h.c_mirror.end(), c_mirror);
  std::copy(g_g.row_off.begin(), g_g.row_off.end(), row_off);
  std::copy(g_g.term_off.begin(), g_g.term_off.end(), term_off);
  std::copy(g_g.term_pos.begin(), g_g.term_pos.end(), term_pos);
  std::copy(g_g.term_w.begin(), g_g.term_w.end(), term_w);
}
