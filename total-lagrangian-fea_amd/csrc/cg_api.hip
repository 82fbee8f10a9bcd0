// cg_api.hip -- the preconditioned CG of the Newton step: the iteration's enqueue path, its hipGraph replay, residual
// replacement and the trace hook; the linear-solve entry points.  Takes the place of the cuDSS solve of the reference
// (SyncedNewton.cu).
#include "newton_handle.h"
#include "pmg_coef.h"

using namespace tlfea;

// Enqueue CG iteration `it` (parity cur = it & 1 selects the r.z slot pair and, in the fused variant, which of the
// two direction buffers is read).  Everything an iteration needs from the previous one (alpha, beta, Chebyshev
// coefficients) is read from device memory, so iterations >= 1 of either parity are the SAME launch sequence.
// Overlapping partition: ghost layers <= Dr of the CG residual take their owners' values, and the next polynomial's fp32
// start vectors of those rows are formed from them (the owned rows' came out of the update kernel).
static int halo_residual_to_ghosts(tlfea_newton_t s) {
  const int N = s->N, Dr = halo_dr(s);
  const size_t n = 3 * (size_t)N;
  if (Dr < 1) return 0;
  TRY(halo_refresh_f64(s, 0, Dr, 3, s->d_r));
  float* f = s->d_f32;
  launch_cheb32_init(s->stream, s->halo.rows(Dr), f + 6 * n, s->d_r, s->d_sc, precond_eff(s) == 2 ? s->pmg.d_coef : s->d_coef,
                     f, f + 2 * n, f + 4 * n, s->halo.rows(0));
  return 0;
}
static int enqueue_residual_replacement(tlfea_newton_t s, double* d_x);
static int enqueue_cg_iteration_impl(tlfea_newton_t s, double* d_x, bool first, int cur, bool fused, int deg, bool replace);
static int enqueue_cg_iteration(tlfea_newton_t s, double* d_x, bool first, int cur, bool fused, int deg,
                                bool replace = false) {
  s->halo.in_cg = true;
  const int rc = enqueue_cg_iteration_impl(s, d_x, first, cur, fused, deg, replace);
  s->halo.in_cg = false;
  return rc;
}
static int enqueue_cg_iteration_impl(tlfea_newton_t s, double* d_x, bool first, int cur, bool fused, int deg, bool replace) {
  tlfea_t10_t d = s->d;
  const int N = s->N;
  const double* w = s->d_w;
  double* pq_part = part(s, 2);
  double *p_old = s->d_p, *p_new = s->d_p2;
  if (fused && cur) std::swap(p_old, p_new);
  // single-GPU fp32 polynomial: its start vectors come out of the previous iteration's update kernel
  const bool b12 = blk12_now(s);
  const bool fuse_init = deg > 1 && cheb_bits_eff(s) != 64 && !s->ar && !b12;
  // Overlapping partition: the CG recurrences (x, r, p, q) live on the OWNED rows.  Two neighbour exchanges per iteration on
  // this level: layer 1 of the direction z (the SpMV's ghost columns) and layers <= Dr of the updated residual (what the
  // next V-cycle starts from).  The residual of a ghost is its OWNER's, bit for bit: recomputing it redundantly (q = H p on
  // ghost rows) differs by round-off, each rank would precondition its own version of r, and at ||r|| ~ 1e-12 ||b|| that
  // inconsistency stalled the iteration (two config-C slabs: floor 1.6e-12).  Dot products weigh owned DOFs (wown) and
  // are summed over ranks: r.z after the preconditioner, p.q after the SpMV; the r.r slots only when the host tests
  // convergence (pcg()).
  const bool hal = s->halo.on;
  const int Dr = hal ? halo_dr(s) : 0;
  const int Nr = hal ? s->halo.rows(0) : N, Np = hal ? s->halo.rows(1) : N;
  const double* wown = hal ? s->d_w : nullptr;
  if (deg > 1) {
    // polynomial preconditioner: z = Cheb(r), r.z slots -> part(cur)   (deg-1 SpMV launches, no reductions)
    TRY(precond_apply(s, s->d_r, s->d_zv, part(s, cur), fuse_init && !first));
    if ((s->ar && !(s->d_own && cheb_bits_eff(s) != 64)) || hal) TRY(parts_sum(s, part(s, cur)));
    if (hal) TRY(halo_refresh_f64(s, 0, 1, 3, s->d_zv));
  }
  if (s->profiling) (void)hipEventRecord(s->ev[4], s->stream);
  // beta = rz(cur)/rz(1-cur); p = z + beta p; q = H p; partials of p.q
  if (fused) {
    if (s->spmv32_now)
      launch_spmv_dir_dot_f32(s->stream, N, d->inc(), s->d_H32, s->d_zv, p_old, first, part(s, 1 - cur), part(s, cur), p_new,
                              s->d_q, pq_part, true);
    else
      launch_spmv_dir_dot(s->stream, N, d->inc(), s->d_H, s->d_zv, p_old, first, part(s, 1 - cur), part(s, cur), p_new,
                          s->d_q, pq_part, true, s->spmv_nt);
  } else {
    launch_pcg_direction(s->stream, 3 * Np, s->d_zv, first, part(s, 1 - cur), part(s, cur), p_old);
    if (s->mf.now)
      TRY(launch_matfree_product(s, p_old, s->d_q, pq_part));
    else if (s->spmv32_now)
      launch_spmv_dir_dot_f32(s->stream, Nr, d->inc(), s->d_H32, s->d_zv, p_old, first, part(s, 1 - cur), part(s, cur), p_old,
                              s->d_q, pq_part, false, wown);
    else
      launch_spmv_dir_dot(s->stream, Nr, d->inc(), s->d_H, s->d_zv, p_old, first, part(s, 1 - cur), part(s, cur), p_old,
                          s->d_q, pq_part, false, s->spmv_nt, wown);
  }
  if (s->profiling) {
    (void)hipEventRecord(s->ev[5], s->stream);
    (void)hipEventSynchronize(s->ev[5]);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, s->ev[4], s->ev[5]);
    s->stage_ms[6] += ms;
    s->stage_n[6] += deg;  // SpMV launches of this iteration (Chebyshev steps included)
  }
  if (s->ar) TRY(iface_sum(s, s->d_q, 3, pq_part, kNPart));  // boundary rows of q + p.q slots, one collective
  if (hal) TRY(parts_sum(s, pq_part));
  if (deg > 1) {
    // alpha = rz(cur)/pq; x += alpha p; r -= alpha q; r.r slots
    if (fuse_init) {
      const size_t n = 3 * (size_t)N;
      float* f = s->d_f32;  // d, z^, res^ start buffers of cheb_apply and (SDS)^-1
      launch_pcg_update_init32(s->stream, Nr, fused ? p_new : p_old, s->d_q, part(s, cur), pq_part, d_x, s->d_r,
                               part(s, 3), s->d_scal + 3, f + 6 * n, s->d_sc,
                               precond_eff(s) == 2 ? s->pmg.d_coef : s->d_coef, f, f + 2 * n, f + 4 * n, wown);
      if (hal && !replace) TRY(halo_residual_to_ghosts(s));
    } else {
      launch_pcg_update_noz(s->stream, N, w, fused ? p_new : p_old, s->d_q, part(s, cur), pq_part, d_x, s->d_r,
                            part(s, 3), s->d_scal + 3);
    }
    if (s->ar) TRY(parts_sum(s, part(s, 3)));
    if (replace) TRY(enqueue_residual_replacement(s, d_x));
  } else {
    // ... and z = Dinv r with the new r.z slots into part(1-cur)
    launch_pcg_update(s->stream, N, s->d_Dinv, w, fused ? p_new : p_old, s->d_q, part(s, cur), pq_part, d_x, s->d_r,
                      s->d_zv, part(s, 1 - cur), part(s, 3));
    if (s->ar) TRY(parts_sum(s, part(s, 1 - cur), part(s, 3)));  // r.z and r.r slots, one collective
  }
  if (hal) s->halo.n_cg_iters++;
  return 0;
}

// r = b - H x in fp64 on H itself, the r.r slots of the TRUE residual and the next polynomial's start vectors (mixed-
// precision iteration only: s->spmv32_now).  q is free between the update and the next iteration's SpMV.
static int enqueue_residual_replacement(tlfea_newton_t s, double* d_x) {
  tlfea_t10_t d = s->d;
  const int N = s->N;
  const size_t n = 3 * (size_t)N;
  // un-fused form: reads x only; its p.q slots go to the scratch slot array of the norms
  // overlapping partition: x lives on the owned rows; layer 1 comes from its owners for the product
  const int Nr = s->halo.on ? s->halo.rows(0) : N;
  if (s->halo.on) TRY(halo_refresh_f64(s, 0, 1, 3, d_x));
  launch_spmv_dir_dot(s->stream, Nr, d->inc(), s->d_H, d_x, d_x, 1, part(s, 0), part(s, 1), s->d_cd, s->d_q, part(s, 5), false,
                      s->spmv_nt);
  float* f = s->d_f32;
  launch_residual_replace_init32(s->stream, Nr, s->cur_b, s->d_q, s->d_r, part(s, 3), f + 6 * n, s->d_sc,
                                 precond_eff(s) == 2 ? s->pmg.d_coef : s->d_coef, f, f + 2 * n, f + 4 * n,
                                 s->halo.on ? s->d_w : nullptr);
  if (s->halo.on) TRY(halo_residual_to_ghosts(s));
  return 0;
}

void tlfea::cg_graphs_destroy(tlfea_newton_t s) {
  for (auto& g : s->cg_graph)
    if (g) {
      (void)hipGraphExecDestroy(g);
      g = nullptr;
    }
}

// The launch sequences (even / odd iteration, odd iteration followed by a residual replacement) captured once as
// hipGraphs and replayed: one host call per CG iteration instead of deg+2 launches.  On small meshes the kernels last
// 5-10 us and the launch rate of the host is what an iteration costs otherwise.  Single-GPU path only (the multi-GPU
// path calls back into the host between kernels).
static int cg_graphs_prepare(tlfea_newton_t s, double* d_x, bool fused, int deg, int bits) {
  const long key[6] = {deg + 1000 * precond_eff(s) + 100000L * (s->pmg.ok ? pmg_coarse_degree_eff(s) : 0),
                       bits + (s->spmv32_now ? 100000L : 0) + (s->mf.now ? 200000L : 0) + (s->mf.now && s->mf.compact ? 800000L : 0) +
                           (pmg_rop_now(s) ? 400000L : 0) + (fine_matfree_live(s) ? 1600000L : 0),
                       (fused ? 1 : 0) + 2 * (long)(size_t)s->cur_b, (long)(size_t)d_x,
                       // the graphs of the matrix-free fine smoother read no fine copy: one built on demand between two
                       // solves (a read-back, a timing run) must not force a re-capture
                       (s->fmf.now ? 0L : (long)(size_t)s->d_B8) ^ fine_matfree_key(s),
                       // the packed records the captured apply launches read
                       (long)(size_t)s->pmg.vertex.d_B8 ^ (s->mf.now ? 3 * (long)(size_t)s->mf.d_Fp + 5 * (long)(size_t)s->mf.d_gp : 0L) ^
                           (s->fmf.now ? 7 * (long)(size_t)s->fmf.d_F32 + 11 * (long)(size_t)s->fmf.d_g32 : 0L)};
  if (s->cg_graph[0] && std::equal(key, key + 6, s->cg_graph_key)) return 0;
  cg_graphs_destroy(s);
  for (int k = 0; k < (s->spmv32_now ? 3 : 2); k++) {
    hipGraph_t g = nullptr;
    auto& hh = s->halo;
    const double c0[5] = {(double)hh.n_exch, (double)hh.n_allred, hh.bytes_exch, hh.bytes_allred, (double)hh.n_cg_iters};
    HIP_TRY(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_cg_iteration(s, d_x, false, k & 1 ? 1 : (k == 2 ? 1 : 0), fused, deg, k == 2);
    const hipError_t e = hipStreamEndCapture(s->stream, &g);
    {  // nothing ran: the counters go back, the cost of one replay is kept
      const double c1[5] = {(double)hh.n_exch, (double)hh.n_allred, hh.bytes_exch, hh.bytes_allred, (double)hh.n_cg_iters};
      for (int t = 0; t < 5; t++) hh.graph_cost[k][t] = c1[t] - c0[t];
      hh.n_exch_cg -= (long)(c1[0] - c0[0]);
      hh.n_allred_cg -= (long)(c1[1] - c0[1]);
      hh.n_exch = (long)c0[0]; hh.n_allred = (long)c0[1]; hh.bytes_exch = c0[2]; hh.bytes_allred = c0[3]; hh.n_cg_iters = (long)c0[4];
      s->n_collectives -= (long)(c1[1] - c0[1]);
    }
    if (rc) return rc;
    HIP_TRY(e);
    HIP_TRY(hipGraphInstantiate(&s->cg_graph[k], g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
  }
  std::copy(key, key + 6, s->cg_graph_key);
  return 0;
}

// Test hook tlfea_newton_cg_trace: record `rec` (0: after launch_pcg_init, j: after iteration j - 1) of the running solve.
// Drains the stream and copies x, r, z, the direction of this iteration (d_p_now: whichever of d_p / d_p2 holds it; null
// before the first iteration) and q, the device's own totals of the slot arrays r.z (both parities), p.q and r.r, and the
// raw slot arrays (r.z even, r.z odd, p.q, r.r, b.b).
constexpr int kCgTraceForm = 24;
static int cg_trace_record(tlfea_newton_t s, int rec, const double* d_x, const double* d_p_now) {
  auto& tr = *s->trace;
  const size_t n = 3 * (size_t)s->N;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  double* v = tr.vecs + (size_t)rec * 5 * n;
  const double* src[5] = {d_x, s->d_r, s->d_zv, d_p_now, d_p_now ? s->d_q : nullptr};
  for (int k = 0; k < 5; k++) {
    if (src[k]) D2H(v + k * n, src[k], n);
    else std::fill(v + k * n, v + (k + 1) * n, 0.0);
  }
  for (int k = 0; k < 4; k++) {
    launch_sum_parts(s->stream, part(s, k), s->d_scal);
    TRY(fetch_scalar(s, s->d_scal, tr.sums + 4 * (size_t)rec + k));
  }
  D2H(tr.slots + (size_t)rec * 5 * kNPart, s->d_parts, (size_t)5 * kNPart);  // the five arrays pcg() zeroes; the sixth is scratch
  return 0;
}
// ... and what the iterations of this solve launch, from the expressions the launchers themselves evaluate:
// [0] fused [1] lanes [2] non-temporal [3] tiled [4] XCD eighths taken [5] grid of the product [6] graphs replayed
// [7] mixed-precision iteration [8] bit j: iteration j ended with a residual replacement [9] update kernel (0 block-Jacobi
// pcg_update, 1 pcg_update_noz, 2 pcg_update_init32) [10] matrix-free product [11] polynomial degree [12] preconditioner
// [13] bits of the polynomial's matrix [14] 12 x 12 node blocks [15] grid of the update kernel [16] lanes, [17] grid and
// [18] XCD eighths of the fp64 product of a residual replacement [19] TLFEA_XCD_ROWS mode
static void cg_trace_form(tlfea_newton_t s, bool fused, int deg, bool graphs) {
  int* f = s->trace->form;
  const int N = s->N;
  const SpmvForm sf = spmv_form(N, fused, s->spmv_nt, s->spmv32_now), rf = spmv_form(N, false, s->spmv_nt, false);
  const bool fuse_init = deg > 1 && cheb_bits_eff(s) != 64 && !s->ar && !blk12_now(s);  // as enqueue_cg_iteration_impl
  f[0] = sf.fused; f[1] = sf.lanes; f[2] = sf.nt; f[3] = sf.tiled; f[4] = sf.xcd; f[5] = sf.grid;
  f[6] = graphs ? 1 : 0;
  f[7] = s->spmv32_now ? 1 : 0;
  f[9] = deg > 1 ? (fuse_init ? 2 : 1) : 0;
  f[10] = s->mf.now ? 1 : 0;
  f[11] = deg; f[12] = deg > 1 ? precond_eff(s) : 0; f[13] = cheb_bits_eff(s); f[14] = blk12_now(s) ? 1 : 0;
  f[15] = slot_grid_256(f[9] == 1 ? 3 * N : N);
  f[16] = rf.lanes; f[17] = rf.grid; f[18] = rf.xcd; f[19] = sf.xcd_mode;
}

// Solve H x = b on the device (b, x device vectors of 3N).  Standard PCG, block-Jacobi.
int tlfea::pcg(tlfea_newton_t s, const double* d_b, double* d_x, int* iters_out, double* rel_out) {
  s->mf.now = false;
  s->mf.last_mode = 0;
  s->fmf.now = false;
  s->fmf.last = 0;
  TRY(refuse_empty_rows(s, "linear solve"));
  if (s->lin.method == 1) return direct_solve(s, d_b, d_x, iters_out, rel_out);
  tlfea_t10_t d = s->d;
  const int N = s->N;
  StageTimer t(s, 4);
  const double* w = s->d_w;
  const bool lp = cheb_bits_eff(s) != 64;
  if (s->halo.on) {
    if (!lp || cheb_degree_eff(s) <= 1)
      return fail("overlapping partition: needs the polynomial / p-multigrid preconditioner on the scaled low-precision copy "
                  "(cheb_degree > 1, cheb_bits 16 or 32)");
    if (halo_dr(s) + 1 > s->halo.depth)
      return fail("overlapping partition: halo depth " + std::to_string(s->halo.depth) + " is below the " +
                  std::to_string(halo_dr(s) + 1) + " layers the fine level needs");
  }
  TRY(precond_setup(s, d_b, 0));
  HIP_TRY(hipMemsetAsync(s->d_parts, 0, (size_t)5 * kNPart * sizeof(double), s->stream));
  launch_pcg_init(s->stream, N, d_b, s->d_Dinv, w, d_x, s->d_r, s->d_zv, part(s, 0), part(s, 4));
  TRY(parts_sum(s, part(s, 0), part(s, 4)));
  launch_sum_parts(s->stream, part(s, 4), s->d_scal + 1);
  double bb = 0.0;
  TRY(fetch_scalar(s, s->d_scal + 1, &bb));
  if (s->trace) TRY(cg_trace_record(s, 0, d_x, nullptr));
  if (lp && blk12_now(s)) {  // the stream is drained: the flag of this solve's node-block factorisation is final
    int bad = 0;
    HIP_TRY(hipMemcpy(&bad, s->d_blk12_err, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return fail("a 12 x 12 node block of H is not positive definite (H is not SPD)");
  }
  int it = 0;
  double rr = bb;
  if (bb > 0.0) {
    const double target = s->lin.rel_tol * s->lin.rel_tol * bb;
    const bool fused_csr = s->pcg_fused < 0 ? (N <= 200000) : (s->pcg_fused != 0);
    const int deg = cheb_degree_eff(s);
    // matrix-free product (serves the un-fused form: p from the direction kernel); everything before the iteration -- the
    // diagonal, the low-precision copy, the lambda_max estimate, the Galerkin operators -- stays on the CSR H
    s->spmv32_now = s->spmv32_every >= 2 && deg > 1 && lp && !s->ar;
    s->mf.now = matfree_chosen(s);
    s->mf.last_mode = s->mf.now ? 1 : 0;
    if (s->mf.now) TRY(matfree_ensure_buffer(s));
    if (s->mf.now) TRY(matfree_ensure_records(s));
    if (!s->mf.now) TRY(hessian_current(s));  // the iteration's product streams H (before any capture)
    const bool fused = fused_csr && !s->mf.now;
    // an outer iteration costs `deg` SpMV launches: test convergence proportionally more often
    int check_every = std::max(1, s->lin.check_every / deg);
    // Every convergence test drains the launch queue (tens of microseconds: as much as an iteration on a small
    // mesh).  Consecutive Newton iterations need nearly the same number of CG iterations, so after the first solve
    // the tests start four iterations before the previous solve's count and then run every iteration.
    const int bits = cheb_bits_eff(s) + 1000 * precond_eff(s);
    int first_check = check_every;
    if (s->last_outer_iters > 1 && s->last_deg == deg && s->last_bits == bits) {
      // (a few iterations earlier, not one: the count can DROP by more than one between solves -- from the first Newton
      // iteration of a step to the second -- and starting at last - 1 then over-solves for several solves in a row)
      static const int back = std::max(1, env_int("TLFEA_PCG_CHECK_BACK", 4));
      first_check = std::max(1, s->last_outer_iters - back);
      check_every = 1;
    }
    s->last_deg = deg;
    s->last_bits = bits;
    s->lmax_mf_ok = true;  // only this call may take the matrix-free lambda_max product (estimate_lam_max)
    const int rc_setup = precond_setup(s, d_b, 1);
    s->lmax_mf_ok = false;
    if (rc_setup) return rc_setup;
    // hipGraph replay: single GPU, and the overlapping partition when its exchange is the built-in RCCL one (enqueued
    // from C++ on this stream, so the neighbour exchanges and all-reduces are captured with the kernels)
    bool graphs = s->use_graphs && !s->ar && !s->profiling && (!s->halo.on || (s->halo.native && halo_graph_wanted()));
    // a capture that fails with collectives inside (RCCL refusing it) is not fatal: back to eager launches, once
    auto prepare_graphs = [&]() -> int {
      if (!graphs) return 0;
      const int rc = cg_graphs_prepare(s, d_x, fused, deg, bits);
      if (rc == 0 || !s->halo.on) return rc;
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(s->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(s->stream, &g);
        if (g) (void)hipGraphDestroy(g);
      }
      (void)hipGetLastError();
      cg_graphs_destroy(s);
      halo_graph_give_up();
      graphs = false;
      std::fprintf(stderr, "tlfea: hipGraph capture of the partitioned CG iteration failed (%s): eager launches from here on\n",
                   tlfea_last_error());
      return 0;
    };
    // mixed-precision iteration: where the fp32 polynomial path runs (its update kernel writes the start vectors the
    // replacement rewrites), on one GPU
    s->cur_b = d_b;
    s->spmv32_now = s->spmv32_every >= 2 && deg > 1 && lp && !s->ar;
    if (s->spmv32_now) {
      TRY(hessian_current(s));
      if (!s->d_H32) HIP_TRY(hipMalloc((void**)&s->d_H32, (size_t)9 * d->nnz_coef * sizeof(float)));
      launch_to_float(s->stream, (size_t)9 * d->nnz_coef, s->d_H, s->d_H32);
    }
    const int R = s->spmv32_every;
    static const bool pcg_trace = std::getenv("TLFEA_PCG_TRACE") != nullptr;  // tools: test every iteration, print r.z, p.q
    if (pcg_trace) {
      first_check = 1;
      check_every = 1;
    }
    bool r_is_true = !s->spmv32_now;  // the residual vector is b - H x of the fp64 system (not the recurrence's)
    // overlapping partition: the start residual r = b of a ghost is its owner's (grad L is evaluated redundantly on the
    // overlap and differs by round-off)
    if (s->halo.on) TRY(halo_refresh_f64(s, 0, halo_dr(s), 3, s->d_r));
    TRY(prepare_graphs());
    double indefinite = 0.0;
    HIP_TRY(hipMemsetAsync(s->d_scal + 3, 0, sizeof(double), s->stream));
    // p-multigrid converges in 30-45 iterations when its coarse polynomial covers the vertex-level spectrum; far more
    // means the size-based degree is too low for this mesh: raise it (kept for later solves) and start over
    const int kStallIters = 56;
    bool stalled = false;
    int stall_check = (precond_eff(s) == 2 && s->pmg.ok && pmg_coarse_degree_eff(s) < kPmgMaxCoarseDeg) ? kStallIters : 0;
    for (int attempt = 0;; attempt++) {
      while (it < s->lin.max_iter) {
        // r.z slots of iteration `it` live in part(it & 1), the previous ones in the other pair
        const bool replace = s->spmv32_now && it > 0 && (it + 1) % R == 0;  // R is even: always an odd iteration
        if (graphs && it > 0) {
          const int gk = replace ? 2 : (it & 1);
          HIP_TRY(hipGraphLaunch(s->cg_graph[gk], s->stream));
          if (s->halo.on) {
            auto& hh = s->halo;
            const double* c = hh.graph_cost[gk];
            hh.n_exch += (long)c[0]; hh.n_exch_cg += (long)c[0];
            hh.n_allred += (long)c[1]; hh.n_allred_cg += (long)c[1];
            hh.bytes_exch += c[2]; hh.bytes_allred += c[3]; hh.n_cg_iters += (long)c[4];
            s->n_collectives += (long)c[1];
          }
        } else
          TRY(enqueue_cg_iteration(s, d_x, it == 0, it & 1, fused, deg, replace));
        if (s->spmv32_now) {
          r_is_true = replace;
          s->n_replacements += replace ? 1 : 0;
        }
        it++;
        if (s->trace) {  // the hook's max_iter is its k: no test before the last iteration
          if (it == 1) cg_trace_form(s, fused, deg, graphs);
          if (replace) s->trace->form[8] |= 1 << (it - 1);
          TRY(cg_trace_record(s, it, d_x, fused ? (((it - 1) & 1) ? s->d_p : s->d_p2) : s->d_p));
        }
        if ((!s->trace && it >= first_check && (it - first_check) % check_every == 0) || it == s->lin.max_iter ||
            (!s->trace && it == stall_check)) {
          if (s->halo.on) TRY(parts_sum(s, part(s, 3)));  // the r.r slots are summed over ranks only when tested
          launch_sum_parts(s->stream, part(s, 3), s->d_scal + 2);
          TRY(fetch_scalar2(s, s->d_scal + 2, &rr, &indefinite));  // ||r||^2 and the r.z < 0 flag
          if (pcg_trace) {
            double rz = 0.0, pq = 0.0;
            launch_sum_parts(s->stream, part(s, (it - 1) & 1), s->d_scal);
            TRY(fetch_scalar(s, s->d_scal, &rz));
            launch_sum_parts(s->stream, part(s, 2), s->d_scal);
            TRY(fetch_scalar(s, s->d_scal, &pq));
            std::fprintf(stderr, "pcg trace: attempt %d it %d rel %.3e rz %.6e pq %.6e indefinite %g\n", attempt, it,
                         std::sqrt(rr / bb), rz, pq, indefinite);
          }
          if (!(rr > target) && rr == rr && !r_is_true) {
            // the recurrence says converged: the verdict is the fp64 system's -- replace the residual and test that
            TRY(enqueue_residual_replacement(s, d_x));
            s->n_replacements++;
            r_is_true = true;
            if (s->halo.on) TRY(parts_sum(s, part(s, 3)));
            launch_sum_parts(s->stream, part(s, 3), s->d_scal + 2);
            TRY(fetch_scalar2(s, s->d_scal + 2, &rr, &indefinite));
          }
          if (!(rr > target)) break;                       // also leaves on NaN
          if (rr > 1e8 * bb || indefinite != 0.0) break;   // the preconditioner is not positive definite
          if (it >= stall_check && stall_check > 0) {      // p-multigrid far beyond its usual 30-45 iterations
            stalled = true;
            break;
          }
        }
      }
      // A Chebyshev polynomial is positive only up to the upper end of its interval: if the power iteration
      // underestimated lambda_max by more than the safety margin, CG breaks down (NaN or growth).  Widen and redo.
      const bool broke = (rr != rr) || rr > 1e8 * bb || (indefinite != 0.0 && rr > target);
      if (stalled && !broke && (attempt >= 3 || pmg_coarse_degree_eff(s) >= kPmgMaxCoarseDeg)) {
        stalled = false;  // nothing left to raise: keep iterating with what there is
        stall_check = 0;
        continue;
      }
      if ((!broke && !stalled) || deg <= 1 || attempt >= 3) break;
      if (stalled && !broke) {
        s->pmg.kc_boost *= 1.45;
        if (s->verbose)
          std::printf("p-multigrid: %d CG iterations without convergence, coarse polynomial degree raised to %d\n", it,
                      pmg_coarse_degree_eff(s));
        stalled = false;
        stall_check = pmg_coarse_degree_eff(s) < kPmgMaxCoarseDeg ? kStallIters : 0;
        TRY(pmg_coefficients(s));
        TRY(prepare_graphs());
      } else {
        s->lam_safety *= 1.5;  // kept for the following solves: the estimate is systematically low on this mesh
        if (s->verbose) std::printf("PCG breakdown: Chebyshev interval widened to %.3g x lambda_max estimate\n", s->lam_safety);
        TRY(cheb_upload_coefficients(s));
        if (precond_eff(s) == 2) TRY(pmg_coefficients(s));
      }
      launch_pcg_init(s->stream, N, d_b, s->d_Dinv, w, d_x, s->d_r, s->d_zv, part(s, 0), part(s, 4));
      TRY(parts_sum(s, part(s, 0), part(s, 4)));
      if (s->halo.on) TRY(halo_refresh_f64(s, 0, halo_dr(s), 3, s->d_r));
      HIP_TRY(hipMemsetAsync(s->d_scal + 3, 0, sizeof(double), s->stream));
      indefinite = 0.0;
      it = 0;
      rr = bb;
      r_is_true = !s->spmv32_now;
      first_check = std::max(1, s->lin.check_every / deg);
      check_every = first_check;
    }
    s->last_outer_iters = it;
  } else {
    HIP_TRY(hipMemsetAsync(d_x, 0, 3 * (size_t)N * sizeof(double), s->stream));
  }
  HIP_TRY(hipGetLastError());
  t.stop();
  const double rel = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
  if (iters_out) *iters_out = it;
  if (rel_out) *rel_out = rel;
  s->lin_last_rel = rel;
  s->lin_last_ok = rel == rel && rel <= s->lin.rel_tol;
  s->lin_worst_rel = (rel != rel) ? rel : std::max(s->lin_worst_rel, rel);
  s->lin_all_ok = s->lin_all_ok && s->lin_last_ok;
  if (rr != rr) return fail("PCG produced NaN (Hessian not SPD?)");
  // The solve stands in for the reference's cuDSS factor + solve, which aborts on failure: an iterate that missed the
  // tolerance (max_iter, or breakdown after the last interval widening) is not applied unless the caller asked for it.
  if (!s->lin_last_ok && !s->lin.on_unconverged) {
    char msg[256];
    std::snprintf(msg, sizeof msg, "PCG did not converge: ||r||/||b|| = %.3e > rel_tol %.1e after %d iterations (max_iter %d)",
                  rel, s->lin.rel_tol, it, s->lin.max_iter);
    return fail(msg);
  }
  return 0;
}
extern "C" int tlfea_newton_get_linsolve_info(tlfea_newton_t s, int* cheb_degree, int* cheb_bits, int* cheb_vector_bits) {
  if (!s) return fail("null argument");
  if (cheb_degree) *cheb_degree = cheb_degree_eff(s);
  if (cheb_bits) *cheb_bits = cheb_bits_eff(s);
  if (cheb_vector_bits)
    *cheb_vector_bits = (cheb_bits_eff(s) != 64 && (!s->ar || s->d_own || precond_eff(s) == 2)) ? 32 : 64;
  return 0;
}
extern "C" int tlfea_newton_linear_solve(tlfea_newton_t s, const double* b, double* x, int* iters, double* rel_res) {
  TRY(refuse_empty_rows(s, "tlfea_newton_linear_solve"));
  const size_t n = 3 * (size_t)s->N;
  HIP_TRY(hipMemcpy(s->d_b, b, n * sizeof(double), hipMemcpyHostToDevice));
  TRY(pcg(s, s->d_b, s->d_dv, iters, rel_res));
  D2H(x, s->d_dv, n);
  return 0;
}

// Test hook (tests/test_gpu_cg_trace.py): the solver's own iterative solve of H x = b for exactly k <= 8 iterations -- pcg()
// itself with max_iter = k and no convergence test before the last iteration -- with every iterate copied out on the way
// (cg_trace_record, cg_trace_form).  The warm state is left as that solve leaves it.
extern "C" int tlfea_newton_cg_trace(tlfea_newton_t s, const double* b, int k, double* vecs, double* sums, double* slots,
                                     int* form) {
  if (!s || !b || !vecs || !sums || !slots || !form) return fail("tlfea_newton_cg_trace: null argument");
  if (k < 1 || k > 8) return fail("tlfea_newton_cg_trace: k must be 1..8");
  if (!s->d_H) return fail("tlfea_newton_cg_trace: no assembled H");
  TRY(hessian_current(s));  // the hook's iteration is the one on the CSR H
  if (dist_on(s)) return fail("tlfea_newton_cg_trace: not available on a partitioned mesh (set_interface / set_halo is active)");
  if (s->lin.method == 1) return fail("tlfea_newton_cg_trace: method = 1 (sparse direct) has no iteration");
  TRY(refuse_empty_rows(s, "tlfea_newton_cg_trace"));
  const size_t n = 3 * (size_t)s->N;
  HIP_TRY(hipMemcpy(s->d_b, b, n * sizeof(double), hipMemcpyHostToDevice));
  tlfea_newton_s::CgTrace tr;
  tr.k = k; tr.vecs = vecs; tr.sums = sums; tr.slots = slots; tr.form = form;
  std::fill(form, form + kCgTraceForm, 0);
  const auto lin = s->lin;
  s->lin.max_iter = k;
  s->lin.on_unconverged = 1;  // k iterations are not meant to converge
  s->trace = &tr;
  int its = 0;
  double rel = 0.0;
  const int rc = pcg(s, s->d_b, s->d_dv, &its, &rel);
  s->trace = nullptr;
  s->lin = lin;
  if (rc) return rc;
  if (its != k) return fail("tlfea_newton_cg_trace: the solve ended after " + std::to_string(its) + " of " + std::to_string(k) + " iterations");
  return 0;
}

// y = H x for host vectors with the current H (partition-boundary rows summed over ranks)
extern "C" int tlfea_newton_apply_hessian(tlfea_newton_t s, const double* x, double* y) {
  const size_t n = 3 * (size_t)s->N;
  TRY(hessian_current(s));
  HIP_TRY(hipMemcpy(s->d_zv, x, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(s->d_parts, 0, (size_t)5 * kNPart * sizeof(double), s->stream));
  launch_spmv_dir_dot(s->stream, s->N, s->d->inc(), s->d_H, s->d_zv, s->d_p, 1, part(s, 1), part(s, 0), s->d_p2,
                      s->d_q, part(s, 2), true, s->spmv_nt);
  if (s->ar) TRY(iface_sum(s, s->d_q, 3, part(s, 2), kNPart));
  HIP_TRY(hipGetLastError());
  D2H(y, s->d_q, n);
  return 0;
}

// y = H x from the matrix-free pair with the current records (tests); an error where the product is not eligible
extern "C" int tlfea_newton_apply_hessian_matfree(tlfea_newton_t s, const double* x, double* y) {
  if (!s || !x || !y) return fail("null argument");
  if (!s->sparsity_done || !matfree_eligible(s))
    return fail("matrix-free Hessian product: not eligible (needs an assembled H of straight-sided T10 elements with one "
                "St.Venant-Kirchhoff material, one GPU, no linear constraints, no obstacles, and no residual evaluation "
                "since the assembly)");
  const size_t n = 3 * (size_t)s->N;
  HIP_TRY(hipMemcpy(s->d_zv, x, n * sizeof(double), hipMemcpyHostToDevice));
  TRY(matfree_ensure_buffer(s));
  TRY(matfree_ensure_records(s));
  TRY(launch_matfree_product(s, s->d_zv, s->d_q, part(s, 2)));
  HIP_TRY(hipGetLastError());
  D2H(y, s->d_q, n);
  return 0;
}
extern "C" int tlfea_newton_get_spmv_mode(tlfea_newton_t s) { return s ? s->mf.last_mode : -1; }
extern "C" int tlfea_newton_get_linsolve_status(tlfea_newton_t s, double* out4) {
  if (!s || !out4) return fail("null argument");
  out4[0] = s->lin_last_rel;
  out4[1] = s->lin_last_ok ? 1.0 : 0.0;
  out4[2] = s->lin_worst_rel;
  out4[3] = s->lin_all_ok ? 1.0 : 0.0;
  return 0;
}
