// Test shim: exposes the host lists of the solve set-up from the element records (csrc/pmg_host.h: ImageHost,
// build_image_groups, image_mass_table) to ctypes, so that the CPU suite can check them without a GPU.  Built by
// tests/test_setup_records_host.py with g++.
#include "../../total-lagrangian-fea_amd/csrc/pmg_host.h"

static tlfea::PmgHost g_h;
static tlfea::RopHost g_r;
static tlfea::ImageHost g_i;

// conn: column-major [10][E]; off/cols: fine node adjacency (sorted); x, y, z: reference coordinates of the fine nodes.
// sizes: Nc, blocks of R, children, groups, passes, rows, instances, accumulator doubles of the largest group
extern "C" int sr_build(int N, int E, const int* conn, const int* off, const int* cols, const double* x, const double* y,
                        const double* z, int inst_budget, int acc_budget, int* sizes) {
  if (!tlfea::pmg_build(N, E, conn, off, cols, g_h)) return 1;
  if (!tlfea::pmg_restrict_op_build(N, off, cols, g_h, g_r)) return 2;
  if (!tlfea::build_image_groups(E, conn, x, y, z, g_h, g_r, inst_budget, acc_budget, g_i)) return 3;
  sizes[0] = g_r.Nc;
  sizes[1] = g_r.nnz;
  sizes[2] = (int)g_r.ch.size();
  sizes[3] = g_i.rg.G();
  sizes[4] = (int)(g_i.rg.pt.size() / 4);
  sizes[5] = (int)g_i.rg.gr_row.size();
  sizes[6] = g_i.n_inst;
  sizes[7] = g_i.rg.acc_max;
  return 0;
}
extern "C" void sr_fetch_rows(int* par0, int* par1, int* r_off, int* r_cols, int* ch_off, int* ch, float* ch_w, int* ch_row,
                              int* ch_pos, int* id_off, int* id_ch, float* id_w, unsigned short* id_pos) {
  std::copy(g_h.par0.begin(), g_h.par0.end(), par0);
  std::copy(g_h.par1.begin(), g_h.par1.end(), par1);
  std::copy(g_r.off.begin(), g_r.off.end(), r_off);
  std::copy(g_r.cols.begin(), g_r.cols.end(), r_cols);
  std::copy(g_r.ch_off.begin(), g_r.ch_off.end(), ch_off);
  std::copy(g_r.ch.begin(), g_r.ch.end(), ch);
  std::copy(g_r.ch_w.begin(), g_r.ch_w.end(), ch_w);
  std::copy(g_i.ch_row.begin(), g_i.ch_row.end(), ch_row);
  std::copy(g_i.ch_pos.begin(), g_i.ch_pos.end(), ch_pos);
  std::copy(g_i.id_off.begin(), g_i.id_off.end(), id_off);
  std::copy(g_i.id_ch.begin(), g_i.id_ch.end(), id_ch);
  std::copy(g_i.id_w.begin(), g_i.id_w.end(), id_w);
  std::copy(g_i.id_pos.begin(), g_i.id_pos.end(), id_pos);
}
// g_pass_off [G + 1], pt [P][4], gr_info [rows][4], gi_head [inst][2], gi_ent [inst][8]
extern "C" void sr_fetch_groups(int* g_pass_off, int* pt, int* gr_info, int* gi_head, int* gi_ent) {
  const auto& g = g_i.rg;
  std::copy(g.g_pass_off.begin(), g.g_pass_off.end(), g_pass_off);
  std::copy(g.pt.begin(), g.pt.end(), pt);
  std::copy(g.gr_info.begin(), g.gr_info.end(), gr_info);
  std::copy(g.gi_head.begin(), g.gi_head.begin() + 2 * (size_t)g_i.n_inst, gi_head);
  std::copy(g.gi_ent.begin(), g.gi_ent.begin() + 8 * (size_t)g_i.n_inst, gi_ent);
}
extern "C" void sr_mass_table(const double* cm, double* cm4) { tlfea::image_mass_table(cm, cm4); }
