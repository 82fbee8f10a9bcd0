// c32_geometry.h -- launch geometry of the single-precision polynomial step (solver_kernels.hip, launch_cheb32).
//
// Pure host code: no HIP, no environment, no state.  The launcher feeds it the rows and blocks of a level, the resident
// workgroups of the candidate instantiations (the occupancy query, cached per instantiation) and the switches, and
// launches what comes back.  The answer depends on nothing else, so the launches a CG graph bakes in are the ones a later
// capture of the same level would choose again.
//
// Regimes:
//   last       the final step of a polynomial: 1024-thread workgroups, at most kNPart of them (its r.z partials must
//              fit the reduction slots)
//   bandwidth  more rows than `bw_rows`: 256-thread workgroups, a lane group works on two rows at a time, the grid is
//              what is resident at once and every group sweeps its share of the rows
//   latency    1024-thread workgroups, at most kNPart of them, one row per group and trip
//   one-round  a non-final step whose rows ALL have a lane group resident at once: 256-thread workgroups, one row per
//              group, no group loops, the grid is ceil(N / G) however large.  With the rule's lanes (two blocks per
//              lane up front) where that fits; else, on a level of 32-lane rows (more than 48 blocks per row: the
//              third level of the cycle, the case this form was measured on), with half the lanes and FOUR blocks per
//              lane up front where that fits; else not at all.  TLFEA_C32_REGIME=4 forces the half-lane form from 16
//              lanes too (tests).
#pragma once

namespace tlfea {

enum C32Regime { kC32Last = 0, kC32Bandwidth = 1, kC32Latency = 2, kC32OneRound = 3 };

struct C32Geometry {
  int regime = kC32Latency;
  int lanes = 16;           // lanes per row
  int threads = 1024;       // per workgroup
  int upfront = 2;          // blocks per lane whose loads go out before the first use
  int rows_per_group = 1;   // rows a lane group works on at a time
  int grid = 1;             // workgroups
  int resident = 0;         // what the occupancy query answered for the instantiation launched (workgroups on the whole
                            // device; 0 in the slot-capped regimes, which do not ask)
};

// Resident workgroups on the whole device of the candidate instantiations AT THE RULE'S LANE COUNT (c32_rule_lanes), 0
// where a candidate does not exist or its query failed.
struct C32Resident {
  int two_row = 0;    // 256 threads, two rows per group
  int one_full = 0;   // one-round, the rule's lanes, two blocks per lane up front
  int one_half = 0;   // one-round, half the rule's lanes, four blocks per lane up front
};

struct C32Switches {
  int bw_rows = 100000;   // TLFEA_C32_BW_N: more rows than this take the bandwidth regime
  int forced_lanes = 0;   // TLFEA_C32_LANES (8 | 16 | 32): the lane count of every regime; no halving
  int regime = -1;        // TLFEA_C32_REGIME (tools and tests): 1 bandwidth, 2 latency, 3 one-round, 4 one-round with
                          // half the lanes; a forced one-round that does not fit falls back to the automatic choice
  bool boundary = false;  // multi-GPU partition-boundary epilogue in use: the half-lane kernel does not have it
  int slots = 512;        // kNPart
};

// lanes per row of the fp64-vector polynomial step (lp_lanes() in solver_kernels.hip adds the TLFEA_LP_LANES switch)
inline int c32_lp_lanes(int N, long long blocks, int forced_lp_lanes) {
  if (forced_lp_lanes == 8 || forced_lp_lanes == 16 || forced_lp_lanes == 32) return forced_lp_lanes;
  return (double)blocks / (N > 1 ? N : 1) > 48.0 ? 32 : 16;
}
// lanes per row of the single-precision step: two blocks per lane and round; ~15 blocks per row (vertex level) -> 8,
// quadratic tets ~30 -> 16, 48+ (lp_lanes = 32) -> 32
inline int c32_rule_lanes(int N, long long blocks, int lp_lanes, int forced_lanes) {
  if (forced_lanes == 8 || forced_lanes == 16 || forced_lanes == 32) return forced_lanes;
  const double avg = (double)blocks / (N > 1 ? N : 1);
  return lp_lanes >= 32 ? 32 : (avg <= 18.0 ? 8 : 16);
}

inline int c32_ceil_div(int a, int b) { return (a + b - 1) / b; }

// one-round candidate with `lanes` lanes: fits when every row's group is resident at once
inline bool c32_one_round_fits(int N, int lanes, int resident) {
  return N >= 1 && lanes >= 1 && lanes <= 256 && resident >= 1 && c32_ceil_div(N, 256 / lanes) <= resident;
}

inline C32Geometry c32_geometry(int N, int lanes, bool last, const C32Resident& res, const C32Switches& sw) {
  C32Geometry g;
  g.lanes = lanes;
  const int n = N > 1 ? N : 1;
  auto capped = [&](int regime) {
    g.regime = regime;
    g.threads = 1024;
    g.upfront = 2;
    g.rows_per_group = 1;
    g.grid = c32_ceil_div(n, 1024 / lanes);
    if (g.grid > sw.slots) g.grid = sw.slots;
    return g;
  };
  auto two_row = [&]() {
    g.regime = kC32Bandwidth;
    g.threads = 256;
    g.upfront = 2;
    g.rows_per_group = 2;
    g.grid = c32_ceil_div(n, 2 * (256 / lanes));
    g.resident = res.two_row;
    const int cap = res.two_row > 1 ? res.two_row : 1;
    if (g.grid > cap) g.grid = cap;
    return g;
  };
  auto one_round = [&](bool half) {
    g.regime = kC32OneRound;
    g.lanes = half ? lanes / 2 : lanes;
    g.threads = 256;
    g.upfront = half ? 4 : 2;
    g.rows_per_group = 1;
    g.grid = c32_ceil_div(n, 256 / g.lanes);
    g.resident = half ? res.one_half : res.one_full;
    return g;
  };
  if (last) return capped(kC32Last);
  const bool may_halve = !(sw.forced_lanes == 8 || sw.forced_lanes == 16 || sw.forced_lanes == 32) && lanes >= 16;
  const bool fits_full = c32_one_round_fits(N, lanes, res.one_full);
  const bool fits_half = !sw.boundary && may_halve && c32_one_round_fits(N, lanes / 2, res.one_half);
  if (sw.regime == 1) return two_row();
  if (sw.regime == 2) return capped(kC32Latency);
  if (sw.regime == 3 && (fits_full || fits_half)) return one_round(!fits_full);
  if (sw.regime == 4 && fits_half) return one_round(true);
  if (N > sw.bw_rows) return two_row();
  if (fits_full) return one_round(false);
  if (fits_half && lanes == 32) return one_round(true);
  return capped(kC32Latency);
}

}  // namespace tlfea
