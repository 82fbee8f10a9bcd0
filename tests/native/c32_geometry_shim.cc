// C entry points of csrc/c32_geometry.h for tests/test_c32_geometry_host.py (the header is pure host code).
#include "../../total-lagrangian-fea_amd/csrc/c32_geometry.h"

extern "C" int c32_shim_rule_lanes(int N, long long blocks, int forced_lp_lanes, int forced_lanes) {
  return tlfea::c32_rule_lanes(N, blocks, tlfea::c32_lp_lanes(N, blocks, forced_lp_lanes), forced_lanes);
}

// resident3 = resident workgroups of {two-row, one-round full lanes, one-round half lanes} at the rule's lane count;
// switches5 = {bw_rows, forced_lanes, regime, boundary, slots}; out7 = {regime, lanes, threads, upfront, rows per group, grid,
// resident workgroups of the instantiation chosen}
extern "C" void c32_shim_geometry(int N, int lanes, int last, const int* resident3, const int* switches5, int* out6) {
  tlfea::C32Resident r;
  r.two_row = resident3[0];
  r.one_full = resident3[1];
  r.one_half = resident3[2];
  tlfea::C32Switches sw;
  sw.bw_rows = switches5[0];
  sw.forced_lanes = switches5[1];
  sw.regime = switches5[2];
  sw.boundary = switches5[3] != 0;
  sw.slots = switches5[4];
  const tlfea::C32Geometry g = tlfea::c32_geometry(N, lanes, last != 0, r, sw);
  out6[0] = g.regime;
  out6[1] = g.lanes;
  out6[2] = g.threads;
  out6[3] = g.upfront;
  out6[4] = g.rows_per_group;
  out6[5] = g.grid;
  out6[6] = g.resident;
}
