// C entry points of csrc/pmg_coef.h for tests/test_pmg_coef_host.py (the header is pure host code).
#include "../../total-lagrangian-fea_amd/csrc/pmg_coef.h"

extern "C" void pmg_shim_cheb_pairs(double hi, double kappa, int terms, double* out) {
  tlfea::cheb_pairs(hi, kappa, terms, out);
}

extern "C" void pmg_shim_fourth_kind_pairs(double hi, int terms, int optimised, double* pairs, double* betas) {
  tlfea::fourth_kind_pairs(hi, terms, optimised != 0, pairs, betas);
}

static tlfea::PmgTable table_of(const int* shape5) {
  tlfea::PmgTable t;
  t.ks = shape5[0];
  t.ks2 = shape5[1];
  t.kc = shape5[2];
  t.k3 = shape5[3];
  t.levels = shape5[4];
  return t;
}

// shape5 = {ks, ks2, kc, k3, levels}; out6 = {resid, restart, beta, coarse, level3, size}
extern "C" void pmg_shim_offsets(const int* shape5, int* out6) {
  const tlfea::PmgTable t = table_of(shape5);
  out6[0] = t.resid();
  out6[1] = t.restart();
  out6[2] = t.beta();
  out6[3] = t.coarse();
  out6[4] = t.level3();
  out6[5] = t.size();
}

// intervals6 = {hi, kappa} of the fine level, the vertex level, level 3; writes size() doubles
extern "C" void pmg_shim_fill(const int* shape5, int smoother_kind, const double* intervals6, double* out) {
  tlfea::pmg_table_fill(table_of(shape5), smoother_kind, {intervals6[0], intervals6[1]}, {intervals6[2], intervals6[3]},
                        {intervals6[4], intervals6[5]}, out);
}

extern "C" int pmg_shim_poly_degree(int n, int forced, int cap) { return tlfea::pmg_poly_degree(n, forced, cap); }

// out5 = {kPmgMaxKs, kPmgMaxCoarseDeg, kPmgMaxLevel3Deg, kPmgTableCap, kChebMaxDeg}
extern "C" void pmg_shim_constants(int* out5) {
  out5[0] = tlfea::kPmgMaxKs;
  out5[1] = tlfea::kPmgMaxCoarseDeg;
  out5[2] = tlfea::kPmgMaxLevel3Deg;
  out5[3] = tlfea::kPmgTableCap;
  out5[4] = tlfea::kChebMaxDeg;
}
