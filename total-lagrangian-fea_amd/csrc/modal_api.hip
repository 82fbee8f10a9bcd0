// modal_api.hip -- modal analysis: LOBPCG on the pencil (H, M) with the CG's preconditioner, and its test
// hooks.  The reference has no modal solver; the block operations follow tests/modal_np.py.
#include "modal_host.h"
#include "newton_handle.h"

using namespace tlfea;

// ---- modal analysis: the lowest pairs of K phi = omega^2 M phi by LOBPCG on the shifted pencil ------------
// A = K + sigma M is H / h assembled with h = 1 / sqrt(sigma), so the iteration runs on the pencil (H, M) itself:
// H x = nu M x with nu = h (omega^2 + sigma).  M need not be definite (the T10 mass of the 5-point Keast rule is not), so
// the block is kept H-orthonormal and the Rayleigh-Ritz step takes the largest theta = 1 / nu (tests/modal_np.py).

static const int* modal_mask(tlfea_newton_t s) { return pinned_on(s) ? s->d->d_fixed_slot : nullptr; }
static bool modal_has_mass(tlfea_t10_t d) { return d->is_csr_setup && d->d_mval && mass_assembled(d); }
static void modal_product(tlfea_newton_t s, int which, int m, const double* X, int ldx, double* Y, int ldy, const int* mask) {
  tlfea_t10_t d = s->d;
  if (which == 0) launch_spmm_block(s->stream, s->N, m, d->d_off, d->d_cols, s->d_H, X, ldx, Y, ldy, mask);
  else launch_massmm_block(s->stream, s->N, m, d->d_off, d->d_cols, d->d_mval, X, ldx, Y, ldy, mask);
}

static int modal_iterate(tlfea_newton_t s, const tlfea_modal_opts& o, int m, double* omega2, double* modes, double* resid,
                         int* info) {
  const int N = s->N, n = 3 * N, ld = 3 * m, nm = o.n_modes;
  const int* mask = modal_mask(s);
  const double h = s->prm.time_step;
  // Memory of a call: S, HS, MS of 3N x 3m doubles each and R of 3N x m -- 80 m bytes per DOF (2.6 kB at m = 32, 0.7 kB at
  // the default m = 9 of six modes), freed on return.  Scratch of the linear solver that is free between solves is
  // borrowed: d_b (start vector of the lambda_max estimate), d_r / d_zv (one column in, T of it out), and inside T what a
  // CG iteration uses (d_cd, d_cd2, the fp32 work vectors, part(0)).  None of it carries state across solves.
  ModalWork wk;
  double *S, *AS, *MS, *R, *slots, *dG, *dC, *dmu, *dnrm;
  TRY(wk.alloc(&S, (size_t)n * ld)); TRY(wk.alloc(&AS, (size_t)n * ld)); TRY(wk.alloc(&MS, (size_t)n * ld));
  TRY(wk.alloc(&R, (size_t)n * m)); TRY(wk.alloc(&slots, gram_slot_doubles(n, ld, ld)));
  TRY(wk.alloc(&dG, (size_t)2 * 96 * 96)); TRY(wk.alloc(&dC, (size_t)96 * 64)); TRY(wk.alloc(&dmu, 32)); TRY(wk.alloc(&dnrm, 64));
  for (double* b : {S, AS, MS}) HIP_TRY(hipMemsetAsync(b, 0, (size_t)n * ld * sizeof(double), s->stream));
  launch_block_hash(s->stream, n, m, o.seed, mask, S, ld);
  // the preconditioner of this H, from a cold lambda_max estimate started at the block's first column
  launch_block_get_col(s->stream, n, S, ld, 0, s->d_b);
  TRY(precond_setup_whole(s, s->d_b, "tlfea_newton_modal_solve"));
  info[3] = cheb_degree_eff(s) > 1 ? precond_eff(s) : 0;

  std::vector<double> GA, GM, theta, Ck, Cfull, nu(m, 0.0), nrm(2 * (size_t)m, 0.0), hG((size_t)2 * ld * ld);
  auto gram_pair = [&](int k) -> int {  // G_A = S^T AS, G_M = S^T MS over the first k columns, to the host
    launch_gram(s->stream, n, k, k, S, ld, AS, ld, slots, dG);
    launch_gram(s->stream, n, k, k, S, ld, MS, ld, slots, dG + (size_t)k * k);
    HIP_TRY(hipMemcpyAsync(hG.data(), dG, (size_t)2 * k * k * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return 0;
  };
  auto sub = [&](const double* G, int k, const std::vector<int>& idx, std::vector<double>& out) {
    const int kk = (int)idx.size();
    out.resize((size_t)kk * kk);
    for (int a = 0; a < kk; a++)
      for (int b = 0; b < kk; b++) out[(size_t)a * kk + b] = G[(size_t)idx[a] * k + idx[b]];
  };
  auto set_nu = [&]() {
    for (int j = 0; j < m; j++) nu[j] = theta[j] != 0.0 ? 1.0 / theta[j] : 0.0;
  };
  auto combine_all = [&](int k, const std::vector<double>& C, int nz, int nz0, int z0, int z1) -> int {
    HIP_TRY(hipMemcpyAsync(dC, C.data(), (size_t)k * nz * sizeof(double), hipMemcpyHostToDevice, s->stream));
    for (double* b : {S, AS, MS}) launch_block_combine(s->stream, n, k, b, ld, dC, nz, nz0, z0, z1);
    HIP_TRY(hipStreamSynchronize(s->stream));  // C's host copy is reused
    return 0;
  };
  auto products_of_x = [&]() {
    modal_product(s, 0, m, S, ld, AS, ld, mask);
    modal_product(s, 1, m, S, ld, MS, ld, mask);
  };
  // start: Rayleigh-Ritz on the hashed block alone
  products_of_x();
  TRY(gram_pair(m));
  {
    std::vector<int> idx(m);
    for (int j = 0; j < m; j++) idx[j] = j;
    sub(hG.data(), m, idx, GA);
    sub(hG.data() + (size_t)m * m, m, idx, GM);
    if (modal::rayleigh_ritz(m, GA, GM, m, theta, Ck) < m)
      return fail("tlfea_newton_modal_solve: the start block is rank deficient (try another seed or a smaller block)");
    set_nu();
    TRY(combine_all(m, Ck, m, m, 0, 0));
  }
  std::vector<char> conv(m, 0), p_valid(m, 0);
  int it = 0, n_conv = 0;
  bool verified = false;
  for (;;) {
    HIP_TRY(hipMemcpyAsync(dmu, nu.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, s->stream));
    launch_block_residual(s->stream, n, m, AS, MS, ld, dmu, R, m, slots, dnrm);
    HIP_TRY(hipMemcpyAsync(nrm.data(), dnrm, (size_t)2 * m * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    n_conv = 0;
    bool all = true;
    for (int j = 0; j < m; j++) {
      const double rn = std::sqrt(nrm[j]), mn = std::sqrt(nrm[m + j]);
      conv[j] = theta[j] > 0.0 && rn <= o.tol * nu[j] * mn;
      if (j < nm) {
        n_conv += conv[j] ? 1 : 0;
        all = all && conv[j];
      }
    }
    if (all) {
      if (verified) break;
      products_of_x();  // the products kept by recurrence drift: convergence is declared on recomputed ones only
      verified = true;
      continue;
    }
    verified = false;
    if (it == o.max_iter) break;
    it++;
    // W = T R on the unconverged columns, masked, then made H-orthogonal to X
    std::vector<int> idx;
    for (int j = 0; j < m; j++) idx.push_back(j);
    for (int j = 0; j < m; j++) {
      if (conv[j]) {
        launch_block_set_col(s->stream, n, nullptr, mask, S, ld, m + j);
        continue;
      }
      launch_block_get_col(s->stream, n, R, m, j, s->d_r);
      TRY(precond_apply(s, s->d_r, s->d_zv, part(s, 0), false));
      launch_block_set_col(s->stream, n, s->d_zv, mask, S, ld, m + j);
      idx.push_back(m + j);
    }
    for (int j = 0; j < m; j++)
      if (!conv[j] && p_valid[j]) idx.push_back(2 * m + j);
    launch_gram(s->stream, n, m, m, AS, ld, S + m, ld, slots, dG);
    HIP_TRY(hipMemcpyAsync(hG.data(), dG, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    {
      std::vector<double> C((size_t)2 * m * m, 0.0);
      for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) C[(size_t)i * m + j] = -hG[(size_t)i * m + j];
      for (int j = 0; j < m; j++) C[(size_t)(m + j) * m + j] = 1.0;
      HIP_TRY(hipMemcpyAsync(dC, C.data(), C.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
      launch_block_combine(s->stream, n, 2 * m, S, ld, dC, m, m, m, m);
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
    modal_product(s, 0, m, S + m, ld, AS + m, ld, mask);   // the iteration's one product with H and with M
    modal_product(s, 1, m, S + m, ld, MS + m, ld, mask);
    TRY(gram_pair(ld));
    sub(hG.data(), ld, idx, GA);
    sub(hG.data() + (size_t)ld * ld, ld, idx, GM);
    const int k = (int)idx.size();
    if (modal::rayleigh_ritz(k, GA, GM, m, theta, Ck) < m)
      return fail("tlfea_newton_modal_solve: the Rayleigh-Ritz basis lost rank (H not positive definite on the free DOFs?)");
    set_nu();
    // new X = S C and new P = its W and P part, both written in one pass over S, AS, MS
    Cfull.assign((size_t)ld * 2 * m, 0.0);
    for (int a = 0; a < k; a++)
      for (int j = 0; j < m; j++) {
        const double c = Ck[(size_t)a * m + j];
        Cfull[(size_t)idx[a] * 2 * m + j] = c;
        if (idx[a] >= m && !conv[j]) Cfull[(size_t)idx[a] * 2 * m + m + j] = c;  // a locked column keeps no direction
      }
    TRY(combine_all(ld, Cfull, 2 * m, m, 0, 2 * m));
    for (int j = 0; j < m; j++) p_valid[j] = !conv[j];
  }
  info[0] = it;
  info[1] = n_conv;
  for (int j = 0; j < nm; j++) {
    const bool pos = theta[j] > 0.0;
    omega2[j] = pos ? nu[j] / h - o.shift : std::nan("");
    const double rn = std::sqrt(nrm[j]), mn = std::sqrt(nrm[m + j]);
    resid[j] = pos && mn > 0.0 ? rn / (nu[j] * mn) : std::nan("");
    if (modes) {
      // x^T H x = 1 and x^T M x = theta: phi = x / sqrt(theta) has phi^T M phi = 1
      launch_block_get_col(s->stream, n, S, ld, j, s->d_r);
      launch_scale(s->stream, n, pos ? 1.0 / std::sqrt(theta[j]) : 0.0, s->d_r);
      HIP_TRY(hipMemcpyAsync(modes + (size_t)j * n, s->d_r, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipGetLastError());
  if (n_conv < nm) {
    char msg[200];
    std::snprintf(msg, sizeof msg, "tlfea_newton_modal_solve: %d of %d modes converged to tol %.1e in %d iterations", n_conv, nm,
                  o.tol, it);
    return fail(msg);
  }
  return 0;
}

extern "C" int tlfea_newton_modal_solve(tlfea_newton_t s, const tlfea_modal_opts* opts, double* omega2, double* modes,
                                        double* resid, int* info) {
  if (!s || !opts || !omega2 || !resid || !info) return fail("tlfea_newton_modal_solve: null argument");
  tlfea_t10_t d = s->d;
  tlfea_modal_opts o = *opts;
  info[0] = info[1] = info[2] = info[3] = 0;
  if (o.n_modes < 1) return fail("tlfea_newton_modal_solve: n_modes must be at least 1");
  if (!(o.shift > 0.0) || !std::isfinite(o.shift)) return fail("tlfea_newton_modal_solve: shift must be finite and positive");
  if (!(o.tol > 0.0) || o.max_iter < 1) return fail("tlfea_newton_modal_solve: tol must be positive and max_iter at least 1");
  if (o.block_extra < 0) o.block_extra = std::max(0, std::min(std::max(2, o.n_modes / 2), 32 - o.n_modes));
  const int m = o.n_modes + o.block_extra;
  if (m > 32) return fail("tlfea_newton_modal_solve: block size n_modes + block_extra = " + std::to_string(m) + " exceeds 32");
  if (d->mat.eta != 0.0 || d->mat.lamd != 0.0 || d->emat_damp)
    return fail("tlfea_newton_modal_solve: damping is set (eta / lambda_damp != 0, uniform or in the material table): C_vis "
                "would enter the pencil; undamped modes only");
  for (int k = 0; k < d->obs.n; k++)
    if (d->obs.o[k].mu > 0.0)
      return fail("tlfea_newton_modal_solve: obstacle " + std::to_string(k) + " has friction: its tangent depends on the time "
                  "step and on the start-of-step positions, so H / h would not be K + shift M; frictionless obstacles only");
  if (dist_on(s)) return fail("tlfea_newton_modal_solve: not available on a partitioned mesh (set_interface / set_halo is active)");
  if (s->lin.method == 1)
    return fail("tlfea_newton_modal_solve: method = 1 (sparse direct) is refused: the direct solve factorises on every call "
                "and has no solve-only entry; use the iterative method for the modal call");
  if (!d->have_dndu || !modal_has_mass(d))
    return fail("tlfea_newton_modal_solve: needs the mass matrix and its sparsity (CalcDnDuPre, CalcMassMatrix) first");
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  TRY(refuse_empty_rows(s, "tlfea_newton_modal_solve"));
  TRY(sync_constraints(s));
  int n_free = s->N;
  if (pinned_on(s)) {
    std::vector<char> fx(s->N, 0);
    for (int i : d->h_fixed) fx[i] = 1;
    for (char c : fx) n_free -= c;
  }
  if (3 * m > 3 * n_free)
    return fail("tlfea_newton_modal_solve: 3 x block size = " + std::to_string(3 * m) + " exceeds the " +
                std::to_string(3 * n_free) + " free DOFs");
  info[2] = m;
  // what the call must leave as it found it: the time step, the warm-start state of the linear solver
  ModalWork wk;
  LamKeep keep;
  const double h0 = s->prm.time_step;
  TRY(keep.save(s, wk, /*solve_state=*/true));  // cold estimates: the result depends on no earlier solve
  s->prm.time_step = 1.0 / std::sqrt(o.shift);
  int rc = assemble(s, /*fq_fresh=*/false);
  if (!rc) rc = modal_iterate(s, o, m, omega2, modes, resid, info);
  const std::string why = rc ? api_error() : std::string();
  (void)hipStreamSynchronize(s->stream);
  s->prm.time_step = h0;
  keep.restore();
  const int rc2 = assemble(s, /*fq_fresh=*/false);  // H of the caller's time step again
  (void)hipStreamSynchronize(s->stream);
  if (rc) {
    api_error() = why;
    return rc;
  }
  return rc2;
}

// Test hooks: Y = H X (which 0) or (M (x) I3) X (which 1) for a host block [3N][m] with the current H; G = X^T Y
extern "C" int tlfea_newton_modal_apply_block(tlfea_newton_t s, int which, int m, const double* X, double* Y, int apply_mask) {
  if (!s || !X || !Y) return fail("tlfea_newton_modal_apply_block: null argument");
  if (m < 1 || m > 32 || which < 0 || which > 1) return fail("tlfea_newton_modal_apply_block: m must be 1..32, which 0 or 1");
  if (which == 0 && !s->d_H) return fail("tlfea_newton_modal_apply_block: no assembled H");
  if (which == 0) TRY(hessian_current(s));
  if (which == 1 && !modal_has_mass(s->d)) return fail("tlfea_newton_modal_apply_block: no mass matrix");
  const size_t cnt = 3 * (size_t)s->N * m;
  ModalWork wk;
  double *dX, *dY;
  TRY(wk.alloc(&dX, cnt)); TRY(wk.alloc(&dY, cnt));
  HIP_TRY(hipMemcpy(dX, X, cnt * sizeof(double), hipMemcpyHostToDevice));
  modal_product(s, which, m, dX, m, dY, m, apply_mask ? modal_mask(s) : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(Y, dY, cnt * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
// Mean milliseconds of one spmm_block launch (Y = H X, m columns, masked) over `reps` back-to-back launches between one
// hipEvent pair, after one untimed launch (tools/modal_timing.py); X is the hashed start block
extern "C" int tlfea_newton_modal_time_spmm(tlfea_newton_t s, int m, int reps, double* ms_out) {
  if (!s || !ms_out) return fail("tlfea_newton_modal_time_spmm: null argument");
  if (m < 1 || m > 32 || reps < 1) return fail("tlfea_newton_modal_time_spmm: m must be 1..32, reps at least 1");
  if (!s->d_H) return fail("tlfea_newton_modal_time_spmm: no assembled H");
  TRY(hessian_current(s));
  const int n = 3 * s->N;
  ModalWork wk;
  double *dX, *dY;
  TRY(wk.alloc(&dX, (size_t)n * m)); TRY(wk.alloc(&dY, (size_t)n * m));
  launch_block_hash(s->stream, n, m, 0u, modal_mask(s), dX, m);
  modal_product(s, 0, m, dX, m, dY, m, modal_mask(s));
  TRY(time_reps(s->stream, reps, ms_out, [&](int) { modal_product(s, 0, m, dX, m, dY, m, modal_mask(s)); return 0; }));
  HIP_TRY(hipGetLastError());
  return 0;
}
extern "C" int tlfea_newton_modal_gram(tlfea_newton_t s, int p, int q, const double* X, const double* Y, double* G) {
  if (!s || !X || !Y || !G) return fail("tlfea_newton_modal_gram: null argument");
  if (p < 1 || p > 96 || q < 1 || q > 96) return fail("tlfea_newton_modal_gram: p and q must be 1..96");
  const size_t n = 3 * (size_t)s->N;
  ModalWork wk;
  double *dX, *dY, *slots, *dG;
  TRY(wk.alloc(&dX, n * p)); TRY(wk.alloc(&dY, n * q)); TRY(wk.alloc(&slots, gram_slot_doubles((int)n, p, q))); TRY(wk.alloc(&dG, (size_t)p * q));
  HIP_TRY(hipMemcpy(dX, X, n * p * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dY, Y, n * q * sizeof(double), hipMemcpyHostToDevice));
  launch_gram(s->stream, (int)n, p, q, dX, p, dY, q, slots, dG);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(G, dG, (size_t)p * q * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
