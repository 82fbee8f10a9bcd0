// pmg_coef.h -- coefficients of the CG preconditioner's polynomials and the layout of the V-cycle's coefficient table.
//
// Pure host code: no HIP, no environment, no state.  precond_api.hip reads the switches and the lambda_max estimates, this
// header turns them into the pairs (c1, c2) a polynomial step reads at coef[2k]: d' = c1 d + c2 (SDS)^-1 res'.
//
// Table of the cycle (pmg.d_coef), in doubles:
//   [0, 2 ks)            fine smoother: (1/theta, 0), then ks - 1 steps
//   resid()              (0, 0): the residual pass, res^ -= Hs d and nothing else
//   restart()            (0, 1/theta): the post-smoother's first pass
//   beta()               kPmgMaxKs weights of z^ += beta_k d (1 for the first-kind smoother)
//   coarse()             two levels: the vertex-level polynomial, kc pairs
//                        three levels: the vertex-level smoother, ks2 pairs, its (0, 0) and restart pairs, then at
//   level3()             the level-3 polynomial, k3 pairs
#pragma once

#include <algorithm>
#include <cmath>

namespace tlfea {

constexpr int kChebMaxDeg = 64;       // the fine polynomial on its own (lin.cheb_degree)
constexpr int kPmgMaxKs = 12;         // terms of a smoother (fine level, vertex level of three)
constexpr int kPmgMaxCoarseDeg = 64;  // degree of the coarsest level's polynomial; the third level stops 4 short
constexpr int kPmgMaxLevel3Deg = kPmgMaxCoarseDeg - 4;
// doubles of pmg.d_coef; the pinned staging area holds as many behind its 8 scalar words
constexpr int kPmgTableCap = 5 * kPmgMaxKs + 8 + 2 * kPmgMaxCoarseDeg;

// Chebyshev iteration on [hi / kappa, hi] (Saad, Iterative Methods, Alg. 12.1): out[0 .. 2 terms) = (1/theta, 0), then
// (rho_k rho_{k-1}, 2 rho_k / delta)
inline void cheb_pairs(double hi, double kappa, int terms, double* out) {
  const double b = hi, a = b / kappa;
  const double theta = 0.5 * (b + a), delta = 0.5 * (b - a), sigma = theta / delta;
  double rho = 1.0 / sigma;
  out[0] = 1.0 / theta; out[1] = 0.0;
  for (int k = 1; k < terms; k++) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    out[2 * k] = rho_new * rho;
    out[2 * k + 1] = 2.0 * rho_new / delta;
    rho = rho_new;
  }
}

// Fourth-kind Chebyshev smoother (needs lambda_max only), optionally with the optimised weights of Lottes (2022), "Optimal
// polynomial smoothers for multigrid V-cycles" (tabulated up to 4 terms; 1 beyond):
//   d0 = 4/(3 hi) D^-1 r ; d_k = (2k-1)/(2k+3) d_{k-1} + (8k+4)/((2k+3) hi) D^-1 r_k ; z_k = z_{k-1} + beta_k d_{k-1}
// pairs[0 .. 2 terms), betas[0 .. terms).  pairs[1] = beta_1: z^0 = beta_1 d0 (the init kernels read it: 0 would mean 1).
inline void fourth_kind_pairs(double hi, int terms, bool optimised, double* pairs, double* betas) {
  static const double kOpt[4][4] = {{1.12500000000000, 0, 0, 0},
                                    {1.02387287570313, 1.26408905371085, 0, 0},
                                    {1.00842544782028, 1.08867839208730, 1.33753125909618, 0},
                                    {1.00391310427285, 1.04035811188593, 1.14863498546254, 1.38268869241000}};
  for (int k = 0; k < terms; k++) betas[k] = (optimised && terms <= 4) ? kOpt[terms - 1][k] : 1.0;
  pairs[0] = 4.0 / (3.0 * hi);
  pairs[1] = betas[0];
  for (int k = 1; k < terms; k++) {
    pairs[2 * k] = (2.0 * k - 1.0) / (2.0 * k + 3.0);
    pairs[2 * k + 1] = (8.0 * k + 4.0) / ((2.0 * k + 3.0) * hi);
  }
}

// The one statement of the table's layout.  Two levels: ks2 = k3 = 0; three: kc = 0.
struct PmgTable {
  int ks = 1, ks2 = 0, kc = 0, k3 = 0, levels = 2;
  constexpr int resid() const { return 2 * ks; }
  constexpr int restart() const { return 2 * ks + 2; }
  constexpr int beta() const { return 2 * ks + 4; }
  constexpr int coarse() const { return 2 * ks + 4 + kPmgMaxKs; }
  constexpr int coarse_resid() const { return coarse() + 2 * ks2; }  // three levels: the vertex level smooths too
  constexpr int coarse_restart() const { return coarse() + 2 * ks2 + 2; }
  constexpr int level3() const { return levels == 3 ? coarse() + 2 * ks2 + 4 : 0; }
  constexpr int size() const { return levels == 3 ? level3() + 2 * k3 : coarse() + 2 * kc; }
};
static_assert(PmgTable{kPmgMaxKs, 0, kPmgMaxCoarseDeg, 0, 2}.size() <= kPmgTableCap, "two-level table exceeds pmg.d_coef");
static_assert(PmgTable{kPmgMaxKs, kPmgMaxKs, 0, kPmgMaxLevel3Deg, 3}.size() <= kPmgTableCap, "three-level table exceeds pmg.d_coef");
static_assert(2 * kChebMaxDeg <= kPmgTableCap, "the fine polynomial's pairs exceed the staging area");

// A polynomial's interval [hi / kappa, hi]; hi = safety factor x the level's lambda_max estimate
struct PmgInterval { double hi = 0.0, kappa = 1.0; };

// The whole table.  smoother_kind of the FINE smoother: 1 first-kind Chebyshev, 3 fourth kind, 4 fourth kind with the
// optimised weights; the vertex level smooths with the first kind.  `level3` is read with three levels only.
inline void pmg_table_fill(const PmgTable& t, int smoother_kind, PmgInterval fine, PmgInterval vertex, PmgInterval level3,
                           double* out) {
  cheb_pairs(fine.hi, fine.kappa, t.ks, out);
  for (int k = 0; k < kPmgMaxKs; k++) out[t.beta() + k] = 1.0;
  if (smoother_kind != 1) fourth_kind_pairs(fine.hi, t.ks, smoother_kind == 4, out, out + t.beta());
  out[t.resid()] = out[t.resid() + 1] = out[t.restart()] = 0.0;
  out[t.restart() + 1] = out[0];  // first kind: d0' = (SDS)^-1 res^ / theta; fourth: 4/(3 hi) (SDS)^-1 res^
  double* c = out + t.coarse();
  if (t.levels != 3) {
    cheb_pairs(vertex.hi, vertex.kappa, t.kc, c);
    return;
  }
  cheb_pairs(vertex.hi, vertex.kappa, t.ks2, c);
  out[t.coarse_resid()] = out[t.coarse_resid() + 1] = out[t.coarse_restart()] = 0.0;
  out[t.coarse_restart() + 1] = c[0];
  cheb_pairs(level3.hi, level3.kappa, t.k3, out + t.level3());
}

// Degree of a coarse level's polynomial from its node count: the measured optimum grows by about 3.2 per doubling, 12 at
// 2 197 nodes; `forced` > 1 overrides, `cap` bounds either
inline int pmg_poly_degree(int n, int forced, int cap) {
  if (forced > 1) return std::min(forced, cap);
  const double kc = 12.0 + 3.2 * (std::log2((double)std::max(2, n)) - 11.1);
  return std::max(8, std::min(cap, (int)std::lround(kc)));
}

}  // namespace tlfea
