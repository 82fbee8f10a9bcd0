// precond_api.hip -- the preconditioners of the device PCG: the Chebyshev polynomial (fp64, low-precision copy, 12 x 12
// node blocks), the lambda_max estimates and the p-multigrid cycle with its hierarchy, Galerkin levels and matrix-free
// fine smoother; precond_setup / precond_apply, and their read-back and test hooks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "newton_handle.h"
#include "pmg_coef.h"
#include "pmg_host.h"

using namespace tlfea;

// ANCF kinds, one GPU, polynomial preconditioner on the low-precision copy: the copy is that of L^-1 H L^-T with the 12 x 12
// node blocks D12 = L L^T (TLFEA_ANCF_BLOCK12=0 keeps the 3 x 3 scaling).  Needs the pattern to come in complete 4 x 4
// groups of blocks (constraint rows that couple single coefficient vectors break that: then the 3 x 3 form stays).
static bool blk12_on(tlfea_newton_t s) {
  if (s->blk12 >= 0) return s->blk12 == 1;
  tlfea_t10_t d = s->d;
  static const bool wanted = env_flag("TLFEA_ANCF_BLOCK12", true);
  bool ok = wanted && d->kind != kT10 && !dist_on(s) && s->N % 4 == 0 && !d->h_off.empty();
  for (int p = 0; ok && p < s->N / 4; p++) {
    const int o0 = d->h_off[4 * p], deg = d->h_off[4 * p + 1] - o0;
    ok = deg % 4 == 0;
    for (int k = 0; ok && k < deg; k++) {
      const int c = d->h_cols[o0 + k];
      ok = c == (d->h_cols[o0 + (k & ~3)] | (k & 3)) && (d->h_cols[o0 + (k & ~3)] & 3) == 0;
    }
    for (int a = 1; ok && a < 4; a++) {
      const int oa = d->h_off[4 * p + a];
      ok = d->h_off[4 * p + a + 1] - oa == deg && std::equal(d->h_cols.begin() + o0, d->h_cols.begin() + o0 + deg, d->h_cols.begin() + oa);
    }
  }
  s->blk12 = ok ? 1 : 0;
  return ok;
}

// cheb_degree 0 = auto = 24.  The steps of the polynomial stream a quarter of the bytes of a CG iteration (fp16 copy
// of H, fp32 vectors) and need no reductions, so a high degree wins on every mesh size: measured (MI355X, rel 1e-12)
// config B 12/16/20/24/32 -> 5.3/5.1/4.7/4.7/4.8 ms per Newton iteration, config C 555/531/539/513/528 ms, against
// 12.8 ms / 1.3-1.5 s with plain block-Jacobi.  The matching interval ratio kappa grows with the degree.
//
// auto: T10 (the polynomial alone, where no p-multigrid hierarchy exists) degree 24 on [lmax/1600, lmax]; the ANCF kinds
// degree 16 on [lmax/200, lmax] with the 12 x 12 node-block scaling, [lmax/400, lmax] without (config D sweep,
// profiles/r03_sweep_ancf_block12.txt: 140.7 ms at 24/1600 -> 82.8 at 16/400 -> 73.8 with the node blocks)
int tlfea::cheb_degree_eff(tlfea_newton_t s) {
  if (s->lin.cheb_degree > 0) return s->lin.cheb_degree;
  return s->d->kind != kT10 ? 16 : 24;
}
static double cheb_kappa_eff(tlfea_newton_t s) {
  if (s->lin.cheb_kappa > 1.0) return s->lin.cheb_kappa;
  const int deg = cheb_degree_eff(s);
  if (s->d->kind != kT10 && s->lin.cheb_degree <= 0) return blk12_on(s) ? 200.0 : 400.0;
  return deg >= 22 ? 1600.0 : (deg >= 14 ? 800.0 : 400.0);
}

// storage precision of the matrix streamed by the Chebyshev steps: 0 = auto = fp16 (scaled copy, see
// solver_kernels.hip); 64 streams H itself
int tlfea::cheb_bits_eff(tlfea_newton_t s) {
  if (cheb_degree_eff(s) <= 1) return 64;
  return s->lin.cheb_bits == 0 ? 16 : s->lin.cheb_bits;
}

// storage of the FINE level's streamed copy inside the p-multigrid cycle: TLFEA_FINE_BITS=8 (experiment) stores it as
// fp8 e4m3 -- 13 instead of 22 bytes per block in the cycle's four fine passes; the coarser levels keep fp16
static int fine_bits(tlfea_newton_t s) {
  static const int forced = env_int("TLFEA_FINE_BITS", 0);
  const int bits = cheb_bits_eff(s);
  return (forced == 8 && bits == 16 && precond_eff(s) == 2 && !s->ar) ? 8 : bits;
}
C32Level tlfea::fine_c32(tlfea_newton_t s) {
  return C32Level{s->d->nnz_coef, s->d->inc(), s->d_B8, s->d_B1, fine_bits(s), s->d_sc, 0};
}
// One step of a level's single-precision polynomial on its first `rows` rows; the ping-pong partners swap roles.
void tlfea::c32_step(tlfea_newton_t s, const C32Level& L, C32Vecs& v, int rows, const double* coef, const double* d_r,
                     double* d_z, double* rz_part, bool last, C32Bnd bnd) {
  launch_cheb32(s->stream, rows, L.nnz, L.inc, L.B8, L.B1, L.bits, v.Dinv_f, L.sc, v.d, coef, v.d2, v.z, v.z2, v.r, v.r2, d_r,
                d_z, rz_part, last, bnd, L.geo < 0 ? nullptr : s->geo_out(L.geo, last));
  v.swap();
}
// storage of the fine level's low-precision copy, (re)allocated where the width changes; a solver that never converts
// never allocates it (0.75 GB at config C)
static int lp_alloc(tlfea_newton_t s, int bits) {
  if (s->lp_bits_alloc == bits && s->d_B8) return 0;
  if (s->d_B8) (void)hipFree(s->d_B8);
  if (s->d_B1) (void)hipFree(s->d_B1);
  s->d_B8 = s->d_B1 = nullptr;
  s->lp_bits_alloc = 0;
  const size_t eb = std::max(1, bits / 8);
  HIP_TRY(hipMalloc(&s->d_B8, (size_t)s->d->nnz_coef * 8 * eb));
  HIP_TRY(hipMalloc(&s->d_B1, (size_t)s->d->nnz_coef * eb));
  s->lp_bits_alloc = bits;
  return 0;
}
// the conversion itself: the copy of the H on the device with the d_sc and d_D of the last stage-0 set-up
static int lp_convert(tlfea_newton_t s) {
  const int bits = fine_bits(s);
  TRY(lp_alloc(s, bits));
  const bool local = s->ar && s->d_own;  // rank-local preconditioner on the owned nodes
  TRY(hessian_current(s));
  launch_lp_convert(s->stream, s->N, s->d->inc(), s->d_H, s->d_sc, local ? s->d_own : nullptr, s->d_D, s->d_B8, s->d_B1,
                    bits);
  HIP_TRY(hipGetLastError());
  s->lp_current = true;
  s->lp_converts++;
  return 0;
}
// Whoever reads the stored copy calls this first: converts where the set-up deferred it and nothing has converted since.
// No-op without a low-precision set-up on the device (nothing to convert from) and under the 12 x 12 form (never deferred).
int tlfea::ensure_fine_copy(tlfea_newton_t s) {
  if (s->lp_current || !s->lp_scaled || fine_bits(s) == 64) return 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return fail("the fine level's low-precision copy is stale inside a stream capture (a set-up must convert it before)");
  return lp_convert(s);
}

// Block-Jacobi scaling of the fine level from the current block diagonal (d_D, d_Dinv must be current) and, unless
// `defer`, the low-precision copy of the current H.  defer: this set-up can still choose the fine smoother from the element
// records, which reads no copy; whoever does read it converts on demand (ensure_fine_copy).
static int lp_build(tlfea_newton_t s, bool defer) {
  tlfea_t10_t d = s->d;
  const int bits = fine_bits(s);
  s->lp_scaled = s->lp_current = false;
  if (bits == 64) return 0;
  if (blk12_now(s)) {
    TRY(lp_alloc(s, bits));
    if (!s->d_L12inv) {
      HIP_TRY(hipMalloc((void**)&s->d_L12inv, (size_t)36 * s->N * sizeof(double)));  // 144 per node of 4 coefficient vectors
      HIP_TRY(hipMalloc((void**)&s->d_L12inv_f, (size_t)36 * s->N * sizeof(float)));
      HIP_TRY(hipMalloc((void**)&s->d_blk12_err, sizeof(int)));
    }
    TRY(hessian_current(s));
    // the flag reports this factorisation alone: a non-SPD block of an earlier H (a rolled-back trial step) must not
    // refuse the solves on the H that followed it
    HIP_TRY(hipMemsetAsync(s->d_blk12_err, 0, sizeof(int), s->stream));
    launch_blk12_factor(s->stream, s->N / 4, d->inc(), s->d_H, s->d_L12inv, s->d_L12inv_f, s->d_sc, s->d_Dinv_s, s->d_blk12_err);
    launch_lp_convert12(s->stream, s->N, d->inc(), s->d_H, s->d_L12inv, s->d_B8, s->d_B1, bits);
    launch_to_float(s->stream, (size_t)9 * s->N, s->d_Dinv_s, s->d_f32 + (size_t)18 * s->N);
    HIP_TRY(hipGetLastError());
    s->lp_current = true;  // (lp_scaled stays false: the 3 x 3 conversion cannot rebuild this copy)
    s->lp_converts++;
    return 0;
  }
  launch_lp_scale(s->stream, s->N, s->d_D, s->d_Dinv, s->d_sc, s->d_Dinv_s);
  s->lp_scaled = true;
  const bool local = s->ar && s->d_own;
  if (!defer) TRY(lp_convert(s));
  if (local) launch_mask_scale(s->stream, s->N, s->d_sc, s->d_own, s->d_sc_mask);
  if (!s->ar || local || precond_eff(s) == 2)
    launch_to_float(s->stream, (size_t)9 * s->N, s->d_Dinv_s, s->d_f32 + (size_t)18 * s->N);
  HIP_TRY(hipGetLastError());
  return 0;
}

bool tlfea::blk12_now(tlfea_newton_t s) {
  return blk12_on(s) && precond_eff(s) != 2 && cheb_degree_eff(s) > 1 && cheb_bits_eff(s) != 64 && s->lin.method == 0;
}

// lambda_max(D^-1 H) by power iteration (warm-started from the previous solve's vector; H changes little between
// Newton iterations).  Power iteration converges from below, hence the safety factor.
// Rank-local variant: lambda_max of the scaled local block (the fp16/fp32 copy itself), no exchange.
static int estimate_lam_max_local(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  const int N = s->N, n = 3 * N, bits = cheb_bits_eff(s);
  const bool cold = !(s->lam_max_loc > 0.0);
  const int iters = cold ? 16 : 4;
  // start vector: the masked scaling itself (positive on every owned DOF) when cold, else the last iterate
  if (cold) HIP_TRY(hipMemcpyAsync(s->d_eigv, s->d_sc_mask, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  for (int k = 0; k <= iters; k++) {
    if (k > 0) {
      launch_cheb_lp(s->stream, N, d->nnz_coef, d->inc(), s->d_B8, s->d_B1, bits, s->d_Dinv_s, s->d_sc, s->d_eigv,
                     s->d_coef, s->d_cd2, nullptr, nullptr, nullptr, nullptr, s->d_r, nullptr, s->d_q, 2);
      launch_apply_dinv(s->stream, N, s->d_Dinv_s, s->d_q, s->d_eigv);
    }
    launch_norm2(s->stream, s->d_eigv, nullptr, n, part(s, 5), s->d_scal);
    launch_scale_inv_sqrt(s->stream, n, s->d_scal, s->d_eigv);
  }
  double ss = 0.0;
  TRY(fetch_scalar(s, s->d_scal, &ss));
  if (!(ss > 0.0)) return fail("lambda_max estimate failed");
  s->lam_max_loc = std::sqrt(ss) * env_double("TLFEA_CHEB_LMAX_SCALE", 1.0);
  s->lam_max = s->lam_max_loc;
  return 0;
}

// TLFEA_LMAX_MATFREE: 1 (default) = the fine power iteration's product runs through the matrix-free pair in
// the solves whose CG iteration does, 0 = always the CSR product.  Read once per process.
static bool lmax_matfree_env() {
  static const bool on = env_flag("TLFEA_LMAX_MATFREE", true);
  return on;
}

static int estimate_lam_max(tlfea_newton_t s, const double* d_b) {
  s->lmax_used_mf = false;
  if (s->ar && s->d_own && cheb_bits_eff(s) != 64) return estimate_lam_max_local(s);
  tlfea_t10_t d = s->d;
  const int N = s->N;
  const bool cold = !(s->lam_max > 0.0);
  // warm: H moves little between Newton iterations and the vector is kept, so the power iteration simply continues across
  // solves -- one product per solve (each is a full fp64 SpMV: 0.7 ms at config C)
  static const int warm_its = std::max(1, env_int("TLFEA_LMAX_WARM_ITERS", 1));
  const int iters = cold ? 16 : warm_its;
  // v <- D^-1 H v / ||D^-1 H v||, the norm stays on the device between iterations: one host read at the end
  // overlapping partition: the iteration lives on the owned rows; ghost layer 1 of the vector is refreshed before every
  // product, deeper ghosts are never touched
  const int Nr = s->halo.on ? s->halo.rows(0) : N, nr = 3 * Nr;
  if (cold) launch_apply_dinv(s->stream, Nr, s->d_Dinv, d_b, s->d_eigv);
  TRY(device_sumsq_async(s, s->d_eigv, s->d_w, nr));
  launch_scale_inv_sqrt(s->stream, nr, s->d_scal, s->d_eigv);
  const bool b12 = blk12_now(s);  // lambda_max of L^-1 H L^-T: v <- L^-1 H L^-T v
  // inside pcg(), in a solve whose iteration runs the matrix-free product: the same product here (0.30 against 0.78 ms
  // at config C).  Every other caller, the partitioned paths and the 12 x 12 scaling keep the CSR product.
  const bool mf = s->lmax_mf_ok && s->mf.now && s->mf.d_ybuf && lmax_matfree_env() && !b12 && !s->ar && !s->halo.on;
  s->lmax_used_mf = mf;
  if (!mf) TRY(hessian_current(s));
  for (int k = 0; k < iters; k++) {
    TRY(halo_refresh_f64(s, 0, 1, 3, s->d_eigv));
    if (b12) launch_blk12_apply(s->stream, N / 4, s->d_L12inv_f, true, s->d_eigv, s->d_cd);
    const double* vv = b12 ? s->d_cd : s->d_eigv;
    if (mf)
      TRY(launch_matfree_product(s, vv, s->d_q, part(s, 2)));
    else
      launch_spmv_dir_dot(s->stream, Nr, d->inc(), s->d_H, vv, vv, 1, part(s, 1), part(s, 0), s->d_p2, s->d_q,
                          part(s, 2), false, s->spmv_nt);
    if (s->ar) TRY(iface_sum(s, s->d_q, 3));
    if (b12) launch_blk12_apply(s->stream, N / 4, s->d_L12inv_f, false, s->d_q, s->d_eigv);
    else launch_apply_dinv(s->stream, Nr, s->d_Dinv, s->d_q, s->d_eigv);
    TRY(device_sumsq_async(s, s->d_eigv, s->d_w, nr));
    launch_scale_inv_sqrt(s->stream, nr, s->d_scal, s->d_eigv);
  }
  double ss = 0.0;
  TRY(fetch_scalar(s, s->d_scal, &ss));
  const double lam = std::sqrt(ss);
  if (!(lam > 0.0)) {
    if (ss == 0.0) return 0;  // zero start vector (b = 0): keep the previous estimate
    return fail("lambda_max estimate failed");
  }
  // TLFEA_CHEB_LMAX_SCALE (tests only): scales the estimate to exercise the breakdown recovery in pcg()
  const double fudge = env_double("TLFEA_CHEB_LMAX_SCALE", 1.0);
  s->lam_max = lam * fudge;
  return 0;
}

// Chebyshev coefficients of this solve to the device: coef[0] = 1/theta, step k reads coef[2k], coef[2k+1].  They live
// in device memory (not kernel arguments) so that the captured launch sequence stays valid when lambda_max moves.
int tlfea::cheb_upload_coefficients(tlfea_newton_t s) {
  const int deg = cheb_degree_eff(s);
  double* h = s->h_pin + 8;
  cheb_pairs(s->lam_safety * s->lam_max, cheb_kappa_eff(s), deg, h);
  HIP_TRY(hipMemcpyAsync(s->d_coef, h, (size_t)2 * deg * sizeof(double), hipMemcpyHostToDevice, s->stream));
  return 0;
}

// z = p_deg(D^-1 H) D^-1 r on [lmax/kappa, lmax]; the last step leaves the r.z slots in rz_part
static int cheb_apply(tlfea_newton_t s, const double* d_r, double* d_z, double* rz_part, bool init_done = false) {
  tlfea_t10_t d = s->d;
  const int N = s->N, deg = cheb_degree_eff(s);
  double *d_old = s->d_cd, *d_new = s->d_cd2;
  const int bits = cheb_bits_eff(s);
  const bool lp = bits != 64;
  const double* Dinv = lp ? s->d_Dinv_s : s->d_Dinv;
  const double* sc = lp ? s->d_sc : nullptr;
  const bool local = s->ar && s->d_own;
  if (lp) TRY(ensure_fine_copy(s));  // every step below streams the stored copy
  if (lp && (!s->ar || local)) {
    // single GPU, or rank-local on the owned nodes: the whole polynomial in single precision (cheb32_kernel); d, z,
    // res ping-pong so that a row's stores never order against loads of other rows; the last step returns
    // z = S z^ in fp64 and the r.z slots.  Rank-local: the masked scaling zeroes r and z on nodes another rank owns.
    C32Level L = fine_c32(s);
    if (local) L.sc = s->d_sc_mask;
    C32Vecs f(s->d_f32, 3 * (size_t)N);
    // init_done: the previous iteration's update kernel already wrote the start vectors (pcg_update_init32_kernel)
    // overlapping partition (meshes without a p-multigrid hierarchy): owned rows only, the direction's first ghost layer
    // is refreshed before every step
    const bool hal = s->halo.on;
    const int Nr = hal ? s->halo.rows(0) : N;
    const C32Bnd bnd = hal ? C32Bnd{nullptr, nullptr, s->d_w} : C32Bnd();
    if (!init_done) launch_cheb32_init(s->stream, Nr, f.Dinv_f, d_r, L.sc, s->d_coef, f.d, f.z, f.r);
    for (int k = 1; k < deg; k++) {
      if (hal) TRY(halo_refresh_f32(s, 0, 1, 3, f.d));
      c32_step(s, L, f, Nr, s->d_coef + 2 * k, d_r, d_z, rz_part, k == deg - 1, bnd);
    }
    // every node's z comes from its owner (zero elsewhere), r.z = sum over owners: one collective for both
    if (local) TRY(iface_sum(s, d_z, 3, rz_part, kNPart));
    return 0;
  }
  // multi-GPU LP path: fp64 vectors, q = Hs d summed over ranks between the SpMV and the vector update
  double *z_cur = d_z, *z_alt = s->d_cz2;
  double *res_cur = s->d_cres, *res_alt = s->d_cres2;
  launch_cheb_init(s->stream, N, Dinv, d_r, sc, s->d_coef, d_old, z_cur, res_cur);
  for (int k = 1; k < deg; k++) {
    const double* coef = s->d_coef + 2 * k;
    const bool last = (k == deg - 1);
    if (s->ar) {
      if (lp)
        launch_cheb_lp(s->stream, N, d->nnz_coef, d->inc(), s->d_B8, s->d_B1, bits, Dinv, sc, d_old, coef, d_new,
                       nullptr, nullptr, nullptr, nullptr, d_r, s->d_w, s->d_q, 2);
      else
        launch_spmv_dir_dot(s->stream, N, d->inc(), s->d_H, d_old, d_old, 1, part(s, 1), part(s, 0), s->d_p2, s->d_q,
                            part(s, 2), false, s->spmv_nt);
      TRY(iface_sum(s, s->d_q, 3));
      launch_cheb_update(s->stream, N, Dinv, s->d_q, d_old, coef, d_new, d_z, s->d_cres, d_r, s->d_w, sc, rz_part,
                         last);
    } else if (lp) {
      double* z_out = last ? d_z : z_alt;
      launch_cheb_lp(s->stream, N, d->nnz_coef, d->inc(), s->d_B8, s->d_B1, bits, Dinv, sc, d_old, coef, d_new, z_cur,
                     z_out, res_cur, res_alt, d_r, s->d_w, rz_part, last ? 1 : 0);
      if (!last) {
        z_alt = z_cur;
        z_cur = z_out;
        std::swap(res_cur, res_alt);
      }
    } else {
      launch_cheb_step(s->stream, N, d->inc(), s->d_H, s->d_Dinv, d_old, coef, d_new, d_z, s->d_cres, d_r, s->d_w,
                       rz_part, last);
    }
    std::swap(d_old, d_new);
  }
  return 0;
}

// ---- two-level p-multigrid preconditioner (T10 quadratic tets -> their linear vertex mesh) ----------------------
// z = M^-1 r, one symmetric V-cycle in the scaled single-precision space of the polynomial path:
//   pre-smooth   2-term Chebyshev polynomial of the fine operator on [lmax/kappa_s, lmax]     (2 fine passes)
//   restrict     r_c = P^T (r - H z)              coarse system Hc = P^T H P (Galerkin, rebuilt every Newton iteration)
//   coarse       degree-kc Chebyshev polynomial of Hc (its own fp16 copy, 1/14 of the fine blocks)
//   prolong      z += P e_c
//   post-smooth  the same 2-term polynomial on the updated residual                           (2 fine passes)
// Every piece is a fixed polynomial / linear map, so M^-1 is a fixed SPD operator and plain CG applies.  Against the
// degree-24 polynomial it replaces: 4 fine + ~1.1 fine-equivalent coarse passes per CG iteration instead of 23, and
// iteration counts that grow slowly with the mesh (CPU prototype: 10k elements 38 vs 33, 83k elements 47 vs 65).
// The coarse problem is solved by a fixed polynomial, so its degree must grow with the coarse mesh: measured optimum
// (kc, kappa_c) = (12, 200) at 2 197 coarse nodes (config B: 3.9 ms), (32, 1600) at 172 081 (config C: 98 ms; 16/400
// gives 159 ms, 48/3200 108 ms) -- about 3.2 per doubling of the node count, with kappa_c = 1.5 kc^2.  The fine
// smoother stays the 2-term polynomial on [lmax/8, lmax] (kappa_s 5 / 8 / 12: 103 / 98 / 158 ms at config C).
static double pmg_kappa_coarse(int kc) {
  static const double forced = env_double("TLFEA_PMG_KAPPA_C", 0.0);
  return forced > 1.0 ? forced : 1.5 * kc * kc;
}
int tlfea::pmg_coarse_degree_eff(tlfea_newton_t s) {
  static const int forced = env_int("TLFEA_PMG_KC", 0);
  const int n_vertex = (dist_on(s) && s->pmg.Nc_glob > 0) ? s->pmg.Nc_glob : s->pmg.vertex.N;
  const int base = pmg_poly_degree(n_vertex, forced, kPmgMaxCoarseDeg);
  return std::min(kPmgMaxCoarseDeg, (int)std::lround(base * s->pmg.kc_boost));
}
// terms of the fine smoother's Chebyshev polynomial (TLFEA_PMG_KS): pre- and post-smoothing cost ks fine passes each
// (ks - 1 steps + the residual / restart pass).  Two regimes, measured: where the fine passes are what an iteration costs
// (bandwidth regime: config C, 2 is the optimum, profiles/r03_sweep_fine_level.txt) and where every launch costs the same
// few microseconds and the vertex-level polynomial's 10-60 launches dominate (meshes up to ~100 k nodes, the reference's
// real meshes: 4 terms cut res16 from 7.9 to 6.4 ms and the badly graded teapot from 35.7 to 24.6 ms per Newton iteration,
// profiles/r03_real_mesh_timing.txt).  The partitioned solve keeps 2 (the ghost depth it needs grows with ks).
int tlfea::pmg_ks(tlfea_newton_t s) {
  static const int forced = env_int("TLFEA_PMG_KS", 0);
  if (forced >= 1) return std::min(forced, kPmgMaxKs);
  if (dist_on(s)) return 2;
  return s->N <= 100000 ? 4 : (s->N <= 500000 ? 3 : 2);  // 3: M2 (172 k nodes) 10.4 -> 9.7 ms, M3 (402 k) 20.5 -> 19.9 ms; C keeps 2
}
// the smoother's interval [lmax / kappa_s, lmax]: 8 for two terms, 1.5 ks^2 beyond (TLFEA_PMG_KAPPA_S)
static double pmg_kappa_s(tlfea_newton_t s) {
  static const double forced = env_double("TLFEA_PMG_KAPPA_S", 0.0);
  if (forced > 1.0) return forced;
  const int ks = pmg_ks(s);
  return ks <= 2 ? 8.0 : 1.5 * ks * ks;
}
// three levels: the vertex level smooths with ks2 terms (TLFEA_PMG_KS2) -- its table [steps | residual pass | restart]
// sits where the two-level cycle keeps the vertex-level polynomial; the level-3 polynomial follows (pmg_coef.h, PmgTable)
static int pmg_ks2(tlfea_newton_t s) {
  static const int forced = env_int("TLFEA_PMG_KS2", 0);
  if (forced >= 1) return std::min(forced, kPmgMaxKs);
  // measured at config C with aggregates of ~2.2 mean vertex edges: 2 terms -> 80 ms, 4 -> 65, 6 -> 58, 10 -> 58, 12 -> 69.
  // Larger aggregates (the grid of bins is coarsened to keep the replicated level small on many ranks) leave the
  // smoother a wider band: terms in proportion to the aggregate size.
  const double ratio = s->pmg.agg.size_ratio > 0.0 ? s->pmg.agg.size_ratio : 2.2;
  return std::max(6, std::min(kPmgMaxKs, (int)std::lround(2.7 * ratio)));  // (5 terms at 2.0-edge cells: 63.5 ms against 59.0 with 6)
}
static double pmg_kappa_s2(tlfea_newton_t s) {
  static const double forced = env_double("TLFEA_PMG_KAPPA_S2", 0.0);
  const int k = pmg_ks2(s);
  return forced > 1.0 ? forced : 2.5 * k * k;  // 90 at 6 terms (measured optimum 60-100)
}
// Smoother polynomial (TLFEA_PMG_SMOOTHER): 1 = first-kind Chebyshev on [lmax / kappa_s, lmax] (the default),
// 3 = fourth-kind Chebyshev (needs lmax only), 4 = fourth kind with the optimised weights of Lottes (2022),
// "Optimal polynomial smoothers for multigrid V-cycles": the z^ update is weighted, z^_k = z^_{k-1} + beta_k d_{k-1}.
static int pmg_smoother_kind() {
  static const int k = env_int("TLFEA_PMG_SMOOTHER", 1);
  return (k == 3 || k == 4) ? k : 1;
}
// Restriction through the stored operator R = S_c P^T S_f^-1 Hs instead of the fine (0, 0) residual pass (pmg_apply):
// one GPU, first-kind smoother, fine copy in 16 or 32 bits, T10 hierarchy with R built.  TLFEA_PMG_RESTRICT_OP=0 keeps
// the residual pass (A/B runs, and the sequence every other configuration runs).
static bool pmg_rop_wanted() {
  static const bool on = env_flag("TLFEA_PMG_RESTRICT_OP", true);
  return on;
}
// The one statement of eligibility, in three stages: what the mesh and the process allow (pmg_prepare builds the lists
// on it), what a set-up builds R for (pmg_build_level), what a cycle or a captured graph runs now (pmg_apply, the key).
static bool pmg_rop_possible(tlfea_newton_t s) {
  return pmg_rop_wanted() && s->d->kind == kT10 && !dist_on(s) && pmg_smoother_kind() == 1;
}
static bool pmg_rop_on(tlfea_newton_t s) {
  if (!pmg_rop_possible(s) || !s->pmg.rop.ok) return false;
  const int fb = fine_bits(s);
  return fb == 16 || fb == 32;
}
bool tlfea::pmg_rop_now(tlfea_newton_t s) { return pmg_rop_on(s) && s->pmg.rop.built; }
// How R is built from H where the fine smoother is matrix-free (DESIGN 3g', 8b): TLFEA_ROP_BUILD=stream (default) reads each
// child's row of H whole through an LDS image of the R row, gather walks the contribution lists.  TLFEA_ROP_STREAM_MAX
// lowers the image's capacity in blocks (tests: rows on both kernels in one build).  Both read once per process.
static bool rop_stream_env() {
  static const bool on = [] {
    const char* e = std::getenv("TLFEA_ROP_BUILD");
    return !(e && std::strcmp(e, "gather") == 0);
  }();
  return on;
}
static int rop_stream_cap() {
  static const int cap = std::max(1, std::min(kRopStreamCap, env_int("TLFEA_ROP_STREAM_MAX", kRopStreamCap)));
  return cap;
}

// ---- fine smoother from the element records (DESIGN 3g') ----------------------------------------------------------------
// TLFEA_PMG_FINE_MATFREE: 0 never, 1 wherever eligible, unset = eligible and at least kFineMatfreeMinRows node rows.  Read once.
static int fine_matfree_env() {
  static const int m = env_tristate("TLFEA_PMG_FINE_MATFREE");
  return m;
}
// Measured on the SVK bars (DESIGN 3g'): 172 k nodes lose 6 % (three smoother terms, and the fp16 copy of that size is
// served from the last-level cache), 402 k gain 8 %, 1.34 M gain 10 %; between 172 k and 402 k nothing was measured, so the
// pick starts just below the smallest size measured to win.
constexpr int kFineMatfreeMinRows = 400000;
// Eligible: where the CG's matrix-free product is (compact rows), inside the p-multigrid cycle with the restriction through
// the stored operator and the first-kind smoother, on one GPU, with the fine storage left at auto.  TLFEA_SPMV_MATFREE does
// not enter: forcing the CG's product on a small mesh leaves the smoother on the low-precision copy.
static double fine_matfree_m0(tlfea_newton_t s) {  // the material scalars are divided by their largest
  const MatfreeCoef& mc = s->mf.mc;
  return std::max(std::max(std::fabs(mc.a), std::fabs(mc.b)), std::max(std::fabs(mc.c1), std::fabs(mc.cl)));
}
// Everything of the choice that stage 0 of a set-up already knows: all but R having been built (pmg_prepare and
// pmg_build_level run in stage 1).  Stage 0 defers the fine level's low-precision copy on it.
static bool fine_matfree_possible(tlfea_newton_t s) {
  if (fine_matfree_env() == 0 || !matfree_eligible(s) || !matfree_compact_env()) return false;
  if (cheb_degree_eff(s) <= 1 || precond_eff(s) != 2 || !pmg_rop_possible(s) || pmg_smoother_kind() != 1) return false;
  if (!(fine_matfree_m0(s) > 0.0)) return false;
  if (s->ar || s->halo.on || s->lin.cheb_bits != 0 || fine_bits(s) != 16) return false;
  return fine_matfree_env() == 1 || s->N >= kFineMatfreeMinRows;
}
static bool fine_matfree_chosen(tlfea_newton_t s) { return fine_matfree_possible(s) && pmg_rop_now(s); }
// The choice of a set-up is taken ONCE, by pmg_build_level before it builds R (rop.built already set), with the compact
// lists in place; the build of R and fine_matfree_setup both follow fmf.now.
static int fine_matfree_choose(tlfea_newton_t s) {
  auto& f = s->fmf;
  f.now = fine_matfree_chosen(s);
  if (f.now) {
    TRY(matfree_ensure_buffer(s));
    f.now = s->mf.compact;
  }
  f.last = f.now ? 1 : 0;
  return 0;
}
// The choice of this preconditioner set-up and, where taken, the float copies of the records H was assembled from, the
// normalised scaling and the scalars (FineMatfree, tlfea_internal.h).  After lp_build (d_sc) and pmg_build_level (R).
static int fine_matfree_setup(tlfea_newton_t s) {
  auto& f = s->fmf;
  tlfea_t10_t d = s->d;
  const MatfreeCoef& mc = s->mf.mc;
  const double m0 = fine_matfree_m0(s);
  if (!f.now) return 0;
  const size_t n = 3 * (size_t)s->N;
  const int np = matfree_points(true);
  if (!f.d_g32) {
    TRY(dmalloc(&f.d_g32, mfr_g_len((size_t)d->E)));
    TRY(dmalloc(&f.d_F32, mfr_F_len((size_t)d->E, np)));
    TRY(dmalloc(&f.d_scn, n));
    TRY(dmalloc(&f.d_ss, 1));
    f.g_ok = false;
  }
  // the packed float records (matfree_records.h): g once per affine set-up, F of this assembly
  launch_matfree_pack<float>(s->stream, d->E, np, s->d_Fq, f.g_ok ? nullptr : s->d_gvec, f.d_F32, f.d_g32);
  f.g_ok = true;
  f.gen = s->mf.gen;
  launch_norm2(s->stream, s->d_sc, nullptr, (int)n, part(s, 5), f.d_ss);
  launch_fine_matfree_scale(s->stream, (int)n, s->d_sc, f.d_ss, 1.0 / (double)n, f.d_scn);
  FineMatfree& v = f.v;
  v.mc.a = (float)(mc.a / m0); v.mc.b = (float)(mc.b / m0); v.mc.c1 = (float)(mc.c1 / m0); v.mc.cl = (float)(mc.cl / m0);
  v.mc.w0 = (float)mc.w0; v.mc.w1 = (float)mc.w1;
  v.mc.rho_inv_h = (float)(mc.rho_inv_h / m0);
  for (int q = 0; q < kNQ; q++) {
    v.mc.mw[q] = (float)mc.mw[q];
    for (int k = 0; k < kNN; k++) v.mc.Nq[q][k] = (float)mc.Nq[q][k];
  }
  v.m0 = m0;
  v.pen_m0 = s->mf.penalty / m0;
  v.gvec = f.d_g32; v.Fq = f.d_F32; v.np = np; v.scn = f.d_scn; v.ss = f.d_ss;
  v.inv_n = 1.0 / (double)n;
  v.ybuf = reinterpret_cast<float*>(s->mf.d_ybuf);  // the CG's product and the smoother never overlap: one buffer
  v.fixed_slot = s->mf.fixed; v.nw = s->d_nw;
  HIP_TRY(hipGetLastError());
  return 0;
}
// the scalars the pair's kernels take BY VALUE (a captured graph holds them): part of the CG graphs' key
long tlfea::fine_matfree_key(tlfea_newton_t s) {
  if (!s->fmf.now) return 0;
  const FineMatfree& v = s->fmf.v;
  const double dv[3] = {v.m0, v.pen_m0, v.inv_n};
  const float fv[7] = {v.mc.a, v.mc.b, v.mc.c1, v.mc.cl, v.mc.w0, v.mc.w1, v.mc.rho_inv_h};
  unsigned long long h = 1469598103934665603ULL;  // FNV-1a over the bytes
  auto mix = [&](const void* p, size_t n) {
    for (size_t k = 0; k < n; k++) h = (h ^ ((const unsigned char*)p)[k]) * 1099511628211ULL;
  };
  mix(dv, sizeof dv);
  mix(fv, sizeof fv);
  return (long)h;
}
// this pass may read the float records: chosen at the set-up, and the records are still those of that assembly
bool tlfea::fine_matfree_live(tlfea_newton_t s) { return s->fmf.now && s->mf.valid && s->fmf.gen == s->mf.gen; }
// Third level (rigid-body-mode aggregates below the vertex level): opt-in with TLFEA_PMG_LEVELS=3.  Measured at config C
// it makes a CG iteration 10-12 % cheaper (4 vertex-level steps + a degree-20..32 polynomial on ~20 000 level-3 nodes
// instead of 31 vertex-level steps) and costs 10-17 % more iterations (33-35 instead of 30, whatever the accuracy of
// the level-3 solve or the vertex-level smoothing interval): 79.4-83.1 ms per Newton iteration against 81.3 ms -- no
// gain, so two levels stay the default.  Below: smoother interval of the vertex level when it is not the coarsest,
// degree / interval of the level-3 polynomial.
static int pmg_levels_wanted(int n_vertex) {
  // Round 3: with a 6-term vertex-level smoother (instead of the 2-term one of round 2) the third level pays: 58 ms
  // against 80 ms per Newton iteration at config C, 23 CG iterations instead of 30 (profiles/r03_sweep_pmg3_*.txt).  Default
  // from 20 000 vertex nodes up (below that the cycle is launch-latency-bound and the extra launches cost more than the
  // shorter polynomial saves: config B 2 197 vertices); TLFEA_PMG_LEVELS=2|3 forces either.
  static const int forced = env_int("TLFEA_PMG_LEVELS", 0);
  static const int min_v = env_int("TLFEA_PMG_L3_MIN", 20000);
  if (forced == 2 || forced == 3) return forced;
  return n_vertex >= min_v ? 3 : 2;
}
static int pmg_level3_degree(int n3) {
  static const int forced = env_int("TLFEA_PMG_KC3", 0);
  return pmg_poly_degree(n3, forced, kPmgMaxLevel3Deg);
}
static double pmg_kappa_level3(int kc) {
  static const double forced = env_double("TLFEA_PMG_KAPPA_C3", 0.0);
  return forced > 1.0 ? forced : 1.5 * kc * kc;
}
// shape of the cycle a solve would run now, hence where its coefficients sit in pmg.d_coef
PmgTable tlfea::pmg_table(tlfea_newton_t s) {
  if (s->pmg.agg.ok) return PmgTable{pmg_ks(s), pmg_ks2(s), 0, pmg_level3_degree(s->pmg.agg.lvl.N), 3};
  return PmgTable{pmg_ks(s), 0, pmg_coarse_degree_eff(s), 0, 2};
}

// 1 = Chebyshev polynomial, 2 = p-multigrid.  Auto: p-multigrid wherever it exists (T10, one GPU, low-precision path,
// no general linear constraint rows -- they couple coefficients the vertex hierarchy does not know about).
int tlfea::precond_eff(tlfea_newton_t s) {
  if (s->lin.precond == 1) return 1;
  tlfea_t10_t d = s->d;
  // T10: quadratic tets -> vertex mesh.  ANCF kinds: all coefficients -> position coefficients (pmg_build_ancf), an
  // experiment switch only (TLFEA_PMG_ANCF=1): measured at config D it needs 44-90 CG iterations against the polynomial's
  // 24 and is no faster, so a precond = 2 request on an ANCF mesh keeps the polynomial
  const char* ancf_env = std::getenv("TLFEA_PMG_ANCF");
  const bool kind_ok = d->kind == kT10 || (ancf_env && std::atoi(ancf_env) == 1 && !dist_on(s));
  const bool possible = kind_ok && !(s->ar && s->d_own) && d->cons_mode != 2 && cheb_degree_eff(s) > 1 &&
                        cheb_bits_eff(s) != 64 && !(s->pmg.tried && !s->pmg.ok);
  return possible ? 2 : 1;
}

static int pmg_prepare(tlfea_newton_t s) {
  auto& m = s->pmg;
  if (m.tried) return 0;
  m.tried = true;
  tlfea_t10_t d = s->d;
  PmgHost h;
  const bool built = d->kind == kT10 ? pmg_build(d->N, d->E, d->h_conn.data(), d->h_off.data(), d->h_cols.data(), h)
                                     : pmg_build_ancf(d->N, d->h_off.data(), d->h_cols.data(), h);
  if (!built) {
    if (s->verbose) std::printf("p-multigrid: the mesh is not a conforming T10 mesh, using the polynomial preconditioner\n");
    return 0;
  }
  m.vertex.N = h.Nc;
  m.vertex.nnz = h.nnz_c;
  TRY(upload_vec(&m.d_par0, h.par0)); TRY(upload_vec(&m.d_par1, h.par1));
  TRY(upload_vec(&m.vertex.d_off, h.c_off)); TRY(upload_vec(&m.vertex.d_cols, h.c_cols)); TRY(upload_vec(&m.vertex.d_diagpos, h.c_diagpos));
  TRY(upload_vec(&m.d_cblk_row, h.cblk_row));
  TRY(upload_vec(&m.d_child_off, h.child_off)); TRY(upload_vec(&m.d_child, h.child)); TRY(upload_vec(&m.d_child_w, h.child_w));
  // T10: the row structure of R and the lists of the combine, for every conforming mesh they fit -- whatever the switches,
  // the size and the number of ranks: which kernel sums Hc depends on the mesh alone (DESIGN 3g')
  RopHost ro;
  const bool have_ro = d->kind == kT10 && pmg_restrict_op_build(d->N, d->h_off.data(), d->h_cols.data(), h, ro);
  if (have_ro) {
    auto& r = m.rop;
    auto& g = m.rows;
    GalRowsHost gr;
    g.ok = pmg_galerkin_rows_build(h, ro, gr);
    if (g.ok) {
      r.nnz = ro.nnz;
      r.n_con = ro.n_con;
      TRY(upload_vec(&r.d_off, ro.off)); TRY(upload_vec(&r.d_cols, ro.cols));
      TRY(upload_vec(&r.d_ch_off, ro.ch_off)); TRY(upload_vec(&r.d_ch, ro.ch)); TRY(upload_vec(&r.d_ch_w, ro.ch_w));
      TRY(upload_vec(&r.d_pos_off, ro.pos_off)); TRY(upload_vec(&r.d_con_pos, ro.con_pos));
      TRY(upload_vec(&g.d_row, gr.row_off)); TRY(upload_vec(&g.d_off, gr.term_off));
      TRY(upload_vec(&g.d_pos, gr.term_pos)); TRY(upload_vec(&g.d_w, gr.term_w));
      const std::vector<int> long_rows = pmg_rop_long_rows(ro, rop_stream_cap());
      g.cap = rop_stream_cap();
      g.n_long = (int)long_rows.size();
      TRY(upload_vec(&g.d_long_rows, long_rows));
      int longest = 0;
      for (int I : long_rows) longest = std::max(longest, ro.off[I + 1] - ro.off[I]);
      g.ws_stride = (size_t)9 * longest;
      // at most 64 MB of images: the long rows are few unless TLFEA_ROP_STREAM_MAX makes every row one
      g.ws_rows = g.n_long ? (int)std::min<size_t>((size_t)g.n_long, std::max<size_t>(4, ((size_t)8 << 20) / g.ws_stride)) : 0;
      if (g.n_long) TRY(dmalloc(&g.d_ws, g.ws_stride * (size_t)g.ws_rows));
    }
  }
  if (!m.rows.ok) {  // ANCF, or lists that do not fit: the gather over the contribution lists
    TRY(upload_vec(&m.d_con_off, h.con_off)); TRY(upload_vec(&m.d_con_base, h.con_base)); TRY(upload_vec(&m.d_con_deg, h.con_deg));
    TRY(upload_vec(&m.d_con_w, h.con_w));
  }
  m.n_upper = (int)h.c_upper.size();
  TRY(upload_vec(&m.d_c_upper, h.c_upper)); TRY(upload_vec(&m.d_c_mirror, h.c_mirror));
  const size_t nc = 3 * (size_t)m.vertex.N;
  TRY(m.vertex.alloc_work());
  TRY(dmalloc(&m.d_coef, (size_t)kPmgTableCap));
  m.ok = true;
  if (s->verbose)
    std::printf("p-multigrid: %d fine nodes -> %d vertex nodes, %d coarse blocks (%d gathered from %zu contributions, the rest "
                "mirrored)\n", d->N, m.vertex.N, m.vertex.nnz, m.n_upper, h.con_w.size());
  if (pmg_rop_possible(s)) {
    if (have_ro) {
      auto& r = m.rop;
      if (!m.rows.ok) {
        r.nnz = ro.nnz;
        r.n_con = ro.n_con;
        TRY(upload_vec(&r.d_off, ro.off)); TRY(upload_vec(&r.d_cols, ro.cols));
        TRY(upload_vec(&r.d_ch_off, ro.ch_off)); TRY(upload_vec(&r.d_ch, ro.ch)); TRY(upload_vec(&r.d_ch_w, ro.ch_w));
      }
      TRY(upload_vec(&r.d_con_off, ro.con_off)); TRY(upload_vec(&r.d_con_blk, ro.con_blk));
      TRY(upload_vec(&r.d_con_ord, ro.con_ord));
      // a matrix-free set-up builds R in the pass that sums Hc, unless TLFEA_ROP_BUILD=gather keeps R on its lists
      r.stream_cap = m.rows.ok && rop_stream_env() ? m.rows.cap : 0;
      HIP_TRY(hipMalloc(&r.d_R8, ((size_t)r.nnz + 1) * 8 * sizeof(float)));
      TRY(dmalloc(&r.d_R1, (size_t)r.nnz + 1));
      r.ok = true;
      if (s->verbose)
        std::printf("p-multigrid: restricted fine operator, %d blocks (%.3f of H), %d contributions, %.1f MB\n", r.nnz,
                    (double)r.nnz / std::max(1, d->nnz_coef), r.n_con,
                    (44.0 * r.nnz + 5.0 * r.n_con + 8.0 * ro.ch.size() + 4.0 * m.vertex.N) / 1048576.0);
    }
  }
  if (s->ar) {
    // Multi-GPU: the coarse level inherits the partition.  A vertex node on the partition boundary is a coarse node
    // replicated on the same ranks; every rank flags the exchange slots of ITS boundary vertices, the flags are summed
    // once, and the flagged slots numbered in ascending order give all ranks the same coarse slot numbering.
    const int ng = s->n_if_glob, nl = s->n_if_loc;
    std::vector<double> flag((size_t)std::max(1, ng), 0.0);
    for (int k = 0; k < nl; k++) {
      const int n = s->h_if_node[k];
      if (h.par0[n] == h.par1[n]) flag[s->h_if_slot[k]] = 1.0;
    }
    HIP_TRY(hipMemcpy(s->d_ibuf, flag.data(), flag.size() * sizeof(double), hipMemcpyHostToDevice));
    if (ng > 0) {
      TRY(call_allreduce(s, s->d_ibuf, ng));
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
    HIP_TRY(hipMemcpy(flag.data(), s->d_ibuf, flag.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int> cslot((size_t)std::max(1, ng), -1);
    int nc_glob = 0;
    for (int t = 0; t < ng; t++)
      if (flag[t] > 0.5) cslot[t] = nc_glob++;
    std::vector<int> cn, cs, bs((size_t)m.vertex.N, -1);
    for (int k = 0; k < nl; k++) {
      const int n = s->h_if_node[k];
      if (h.par0[n] != h.par1[n]) continue;
      const int I = h.par0[n];
      cn.push_back(I);
      cs.push_back(cslot[s->h_if_slot[k]]);
      bs[I] = cslot[s->h_if_slot[k]];
    }
    m.n_ifc_loc = (int)cn.size();
    m.n_ifc_glob = nc_glob;
    if (cn.empty()) { cn.push_back(0); cs.push_back(0); }
    TRY(upload_vec(&m.d_ifc_node, cn)); TRY(upload_vec(&m.d_ifc_slot, cs)); TRY(upload_vec(&m.d_bslot_c, bs));
    std::vector<double> wc3(nc);
    for (int I = 0; I < m.vertex.N; I++) {
      const double w = s->h_nw[h.child[h.child_off[I]]];  // the vertex itself is its first child
      wc3[3 * (size_t)I] = wc3[3 * (size_t)I + 1] = wc3[3 * (size_t)I + 2] = w;
    }
    TRY(upload_vec(&m.d_wc3, wc3));
    {
      double cnt = 0.0;
      for (int I = 0; I < m.vertex.N; I++) cnt += wc3[3 * (size_t)I];
      TRY(allreduce_host(s, s->d_ibuf, &cnt, 1));
      m.Nc_glob = (int)std::lround(cnt);
    }
    std::vector<float> cw(h.child_w);
    for (size_t t = 0; t < cw.size(); t++) cw[t] = (float)(cw[t] * s->h_nw[h.child[t]]);
    TRY(upload_vec(&m.d_child_w_dist, cw));
    if (s->verbose) std::printf("p-multigrid: partitioned coarse level, %d of %d boundary vertices on this rank\n", m.n_ifc_loc, nc_glob);
  }
  if (s->halo.on) {
    // Overlapping partition: the coarse level inherits owners and layers (a vertex is adjacent to the vertices of its
    // elements: the same graph distance).  Coarse exchange lists = the fine lists restricted to vertex nodes.
    // (the third level is not partitioned yet: the multi-GPU cycle stays at two levels)
    auto& hl = s->halo;
    const auto& Lf = hl.lv[0];
    auto& Lc = hl.lv[1];
    halo_free_plans(Lc);
    const int P = (int)hl.peers.size();
    auto is_vertex = [&](int n) { return h.par0[n] == h.par1[n]; };
    Lc.send_off.assign(P + 1, 0);
    Lc.recv_off.assign(P + 1, 0);
    Lc.send_nodes.clear(); Lc.send_layer.clear(); Lc.recv_nodes.clear(); Lc.recv_layer.clear();
    for (int k = 0; k < P; k++) {
      for (int t = Lf.send_off[k]; t < Lf.send_off[k + 1]; t++)
        if (is_vertex(Lf.send_nodes[t])) {
          Lc.send_nodes.push_back(h.par0[Lf.send_nodes[t]]);
          Lc.send_layer.push_back(Lf.send_layer[t]);
        }
      for (int t = Lf.recv_off[k]; t < Lf.recv_off[k + 1]; t++)
        if (is_vertex(Lf.recv_nodes[t])) {
          Lc.recv_nodes.push_back(h.par0[Lf.recv_nodes[t]]);
          Lc.recv_layer.push_back(Lf.recv_layer[t]);
        }
      Lc.send_off[k + 1] = (int)Lc.send_nodes.size();
      Lc.recv_off[k + 1] = (int)Lc.recv_nodes.size();
    }
    // owner weights and layer counts of the coarse nodes (coarse ids ascend with the fine ids of their vertices, so the
    // coarse numbering is ordered by layer as well -- checked)
    std::vector<double> wc3(nc);
    std::vector<int> lay_c((size_t)m.vertex.N);
    for (int I = 0; I < m.vertex.N; I++) {
      const int nf = h.child[h.child_off[I]];  // the vertex itself is its first child
      lay_c[I] = hl.layer[nf];
      wc3[3 * (size_t)I] = wc3[3 * (size_t)I + 1] = wc3[3 * (size_t)I + 2] = lay_c[I] == 0 ? 1.0 : 0.0;
      if (I > 0 && lay_c[I] < lay_c[I - 1]) return fail("p-multigrid: coarse numbering is not ordered by ghost layer");
    }
    hl.n_upto_c.assign(hl.depth + 1, 0);
    for (int k = 0; k <= hl.depth; k++) hl.n_upto_c[k] = (int)(std::upper_bound(lay_c.begin(), lay_c.end(), k) - lay_c.begin());
    TRY(upload_vec(&m.d_wc3, wc3));
    double cnt = hl.n_upto_c[0];
    TRY(allreduce_host(s, hl.d_red, &cnt, 1));
    m.Nc_glob = (int)std::lround(cnt);
    if (s->verbose)
      std::printf("p-multigrid: overlapped coarse level, %d owned of %d local vertices (%d over all ranks)\n", hl.n_upto_c[0],
                  m.vertex.N, m.Nc_glob);
  }
  // third level: single GPU (greedy aggregates, or the grid of bins with TLFEA_PMG_AGG=bins) and the overlapping
  // partition (bins: the level is replicated on every rank, see pmg_host.h)
  const bool l3_halo = s->halo.on && s->halo.world > 0;
  if ((!dist_on(s) || l3_halo) && pmg_levels_wanted(s->halo.on ? m.Nc_glob : m.vertex.N) == 3) {
    // reference coordinates of the vertex nodes (slot 0 of a coarse node's children is the vertex itself)
    std::vector<double> xf((size_t)3 * d->N), Xv((size_t)3 * m.vertex.N);
    D2H(xf.data(), d->d_xt, (size_t)d->N);
    D2H(xf.data() + d->N, d->d_yt, (size_t)d->N);
    D2H(xf.data() + 2 * (size_t)d->N, d->d_zt, (size_t)d->N);
    for (int I = 0; I < m.vertex.N; I++) {
      const int n = h.child[h.child_off[I]];
      for (int c = 0; c < 3; c++) Xv[(size_t)c * m.vertex.N + I] = xf[(size_t)c * d->N + n];
    }
    AggHost a;
    auto& g = m.agg;
    // aggregates: the grid of bins everywhere (one cycle on one GPU and on many; measured equal to the greedy aggregates of
    // round 2 at config C: 59.0 vs 58.5 ms); TLFEA_PMG_AGG=greedy keeps those on one GPU
    static const bool bins_env = !(std::getenv("TLFEA_PMG_AGG") && std::string(std::getenv("TLFEA_PMG_AGG")) == "greedy");
    bool built = false;
    if (l3_halo || bins_env) {
      // --- grid of bins.  Agreed numbers: bounding box, mean / longest vertex edge (over owned rows), then the moments ---
      std::vector<char> owned;
      if (s->halo.on) {
        owned.resize((size_t)m.vertex.N);
        for (int I = 0; I < m.vertex.N; I++) owned[I] = s->halo.layer[h.child[h.child_off[I]]] == 0;
      }
      const char* own = s->halo.on ? owned.data() : nullptr;
      double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, sum_len = 0.0, n_len = 0.0, max_len = 0.0;
      for (int I = 0; I < m.vertex.N; I++) {
        if (own && !own[I]) continue;
        for (int c = 0; c < 3; c++) {
          lo[c] = std::min(lo[c], Xv[(size_t)c * m.vertex.N + I]);
          hi[c] = std::max(hi[c], Xv[(size_t)c * m.vertex.N + I]);
        }
        for (int k = h.c_off[I]; k < h.c_off[I + 1]; k++) {
          const int J = h.c_cols[k];
          if (J == I) continue;
          double l2 = 0.0;
          for (int c = 0; c < 3; c++) l2 += (Xv[(size_t)c * m.vertex.N + I] - Xv[(size_t)c * m.vertex.N + J]) * (Xv[(size_t)c * m.vertex.N + I] - Xv[(size_t)c * m.vertex.N + J]);
          const double l = std::sqrt(l2);
          sum_len += l; n_len += 1.0; max_len = std::max(max_len, l);
        }
      }
      double n_own_glob = s->halo.on ? 0.0 : (double)m.vertex.N;
      if (s->halo.on) {
        // gather-by-sum: rank r fills slots [9 r, 9 r + 9) of a zero vector, the all-reduce hands every rank all of them
        const int W = s->halo.world, R = s->halo.rank;
        if (9 * W > 2 * kNPart) return fail("p-multigrid: too many ranks for the level-3 set-up buffer");
        std::vector<double> v((size_t)9 * W, 0.0);
        const double mine[9] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], sum_len, n_len, max_len};
        std::copy(mine, mine + 9, v.begin() + (size_t)9 * R);
        TRY(allreduce_host(s, s->halo.d_red, v.data(), v.size()));
        sum_len = n_len = max_len = 0.0;
        for (int r = 0; r < W; r++) {
          for (int c = 0; c < 3; c++) {
            lo[c] = std::min(lo[c], v[(size_t)9 * r + c]);
            hi[c] = std::max(hi[c], v[(size_t)9 * r + 3 + c]);
          }
          sum_len += v[(size_t)9 * r + 6];
          n_len += v[(size_t)9 * r + 7];
          max_len = std::max(max_len, v[(size_t)9 * r + 8]);
        }
        n_own_glob = (double)m.Nc_glob;
      }
      static const double factor = env_double("TLFEA_PMG_BIN", 2.0);
      static const double max_bins = env_double("TLFEA_PMG_BINS_MAX", 12000.0);
      const double mean_len = n_len > 0.0 ? sum_len / n_len : 1.0;
      BinGrid grid = bin_grid(lo, hi, mean_len, max_len, factor);
      // the replicated level stays small: at most max_bins cells, whatever the number of ranks
      while ((double)grid.cells() > max_bins) grid = bin_grid(lo, hi, mean_len, max_len, (grid.size / mean_len) * 1.1);
      std::vector<int> agg;
      std::vector<double> mom;
      bin_moments(m.vertex.N, Xv.data(), grid, own, agg, mom);
      if (s->halo.on) {
        double* d_m = nullptr;
        TRY(dmalloc(&d_m, mom.size()));
        HIP_TRY(hipMemcpy(d_m, mom.data(), mom.size() * sizeof(double), hipMemcpyHostToDevice));
        TRY(call_allreduce(s, d_m, (int)mom.size()));
        HIP_TRY(hipStreamSynchronize(s->stream));
        HIP_TRY(hipMemcpy(mom.data(), d_m, mom.size() * sizeof(double), hipMemcpyDeviceToHost));
        (void)hipFree(d_m);
      }
      built = agg_build_bins(m.vertex.N, h.c_off.data(), h.c_cols.data(), Xv.data(), grid, agg, mom, own, a);
      g.bins = built;
      g.size_ratio = built ? grid.size / mean_len : 0.0;
      if (s->verbose)
        std::printf("p-multigrid: third level on a %d x %d x %d grid of bins (cell %.3g = %.2f mean vertex edges; %.0f owned vertices "
                    "over all ranks)%s\n", grid.dims[0], grid.dims[1], grid.dims[2], grid.size, grid.size / mean_len, n_own_glob,
                    built ? "" : " -- FAILED, two levels");
      if (s->halo.on) {
        // every rank must take the same branch: agree that ALL built the level
        double okv = built ? 0.0 : 1.0;
        TRY(allreduce_host(s, s->halo.d_red, &okv, 1));
        built = built && okv < 0.5;
      }
    } else {
      built = agg_build(m.vertex.N, h.c_off.data(), h.c_cols.data(), Xv.data(), a);
    }
    if (built) {
      g.Na = a.Na; g.lvl.N = a.N3; g.lvl.nnz = a.nnz3; g.n_pairs = a.n_pairs;
      TRY(upload_vec(&g.d_agg, a.agg)); TRY(upload_vec(&g.d_active, a.active)); TRY(upload_vec(&g.d_rvec, a.rvec));
      TRY(upload_vec(&g.d_mem_off, a.mem_off));
      if (a.mem.empty()) a.mem.push_back(0);
      TRY(upload_vec(&g.d_mem, a.mem));
      TRY(upload_vec(&g.lvl.d_off, a.off3)); TRY(upload_vec(&g.lvl.d_cols, a.cols3)); TRY(upload_vec(&g.lvl.d_diagpos, a.diag3));
      TRY(upload_vec(&g.d_pair_A, a.pair_A)); TRY(upload_vec(&g.d_pair_pos, a.pair_pos)); TRY(upload_vec(&g.d_pair_B, a.pair_B));
      TRY(upload_vec(&g.d_pcon_off, a.pcon_off)); TRY(upload_vec(&g.d_pcon_base, a.pcon_base));
      TRY(upload_vec(&g.d_pcon_deg, a.pcon_deg)); TRY(upload_vec(&g.d_pcon_i, a.pcon_i)); TRY(upload_vec(&g.d_pcon_j, a.pcon_j));
      TRY(g.lvl.alloc_work());
      if (s->halo.on) TRY(dmalloc(&g.d_r3, 3 * (size_t)g.lvl.N));
      g.ok = true;
      if (s->verbose)
        std::printf("p-multigrid: third level, %d aggregates with rigid-body modes (%d nodes, %d blocks)\n", g.Na, g.lvl.N,
                    g.lvl.nnz);
    }
  }
  return 0;
}

// ---- solve set-up from the element records (DESIGN 3g') -----------------------------------------------------------------
// TLFEA_SETUP_RECORDS: 0 never, 1 wherever eligible, unset = eligible and at least kFineMatfreeMinRows node rows (the size
// from which the fine smoother takes the matrix-free form by itself: forcing that smoother on a small mesh does not bring
// this form with it).  Read once.
static int setup_records_env() {
  static const int m = env_tristate("TLFEA_SETUP_RECORDS");
  return m;
}
// Budgets of the coarse rows' groups (build_row_groups4): a vertex row of a tet mesh has ~24 corner instances, so a group
// of 32 instances would hold one row and fill its second pass to a half; 48 pairs two rows into three full passes.
// TLFEA_IMG_INST / TLFEA_IMG_ACC (tools: the sweep of profiles/setup_records.txt).
static int image_inst_budget() {
  static const int v = std::max(16, env_int("TLFEA_IMG_INST", 48));
  return v;
}
static int image_acc_budget() {
  static const int v = std::max(64, env_int("TLFEA_IMG_ACC", 1536));
  return v;
}
// the coarse work lists, the one-child tables and the buffers: once per mesh, after pmg_prepare
static int setup_records_prepare(tlfea_newton_t s) {
  auto& r = s->sr;
  if (r.tried) return 0;
  r.tried = true;
  tlfea_t10_t d = s->d;
  auto& m = s->pmg;
  if (!m.ok || !m.rop.ok || !m.rows.ok || !s->d_cmass) return 0;
  // the hierarchy's host lists are not kept: build them again (integer work, once)
  PmgHost h;
  RopHost ro;
  ImageHost ih;
  if (!pmg_build(d->N, d->E, d->h_conn.data(), d->h_off.data(), d->h_cols.data(), h)) return 0;
  if (!pmg_restrict_op_build(d->N, d->h_off.data(), d->h_cols.data(), h, ro)) return 0;
  const size_t N = (size_t)d->N;
  if (!build_image_groups(d->E, d->h_conn.data(), d->h_X0.data(), d->h_X0.data() + N, d->h_X0.data() + 2 * N, h, ro,
                          image_inst_budget(), image_acc_budget(), ih))
    return 0;
  if (ro.nnz != m.rop.nnz || assemble_affine_lds_max(ih.rg.acc_max) > device_lds_limit()) return 0;
  const std::vector<int>* src[5] = {&ih.rg.g_pass_off, &ih.rg.pt, &ih.rg.gr_info, &ih.rg.gi_head, &ih.rg.gi_ent};
  for (int k = 0; k < 5; k++) {
    TRY(dmalloc(&r.d_rg[k], src[k]->size() + 4));
    HIP_TRY(hipMemcpy(r.d_rg[k], src[k]->data(), src[k]->size() * sizeof(int), hipMemcpyHostToDevice));
  }
  r.rg = RowGroups4{ih.rg.G(), std::max(1, ih.n_inst), ih.rg.acc_max, r.d_rg[0], reinterpret_cast<const int4*>(r.d_rg[1]),
                    reinterpret_cast<const int4*>(r.d_rg[2]), reinterpret_cast<const int2*>(r.d_rg[3]),
                    reinterpret_cast<const int2*>(r.d_rg[4])};
  r.passes = (int)(ih.rg.pt.size() / 4);
  r.n_ch = (int)ih.ch_row.size();
  double cm[160], cm4[64];
  HIP_TRY(hipMemcpy(cm, s->d_cmass, sizeof cm, hipMemcpyDeviceToHost));
  image_mass_table(cm, cm4);
  TRY(dmalloc(&r.d_cmass4, 64));
  HIP_TRY(hipMemcpy(r.d_cmass4, cm4, sizeof cm4, hipMemcpyHostToDevice));
  TRY(upload_vec(&r.d_ch_row, ih.ch_row)); TRY(upload_vec(&r.d_ch_pos, ih.ch_pos));
  TRY(upload_vec(&r.d_id_off, ih.id_off)); TRY(upload_vec(&r.d_id_ch, ih.id_ch));
  TRY(upload_vec(&r.d_id_w, ih.id_w)); TRY(upload_vec(&r.d_id_pos, ih.id_pos));
  TRY(dmalloc(&r.d_img, (size_t)9 * ro.nnz + 9));
  TRY(dmalloc(&r.d_dbuf, (size_t)d->Epad * 6 * kNN));
  r.ok = true;
  if (s->verbose)
    std::printf("set-up from the element records: %d coarse rows in %d groups, %d passes of %d instances, accumulator %d doubles, "
                "image %.1f MB\n", ro.Nc, r.rg.G, r.passes, ih.n_inst, r.rg.acc_max, 72.0 * ro.nnz / 1048576.0);
  return 0;
}
// What the form needs beyond the records being claimed: everything of the solve runs from the records (the CG's product,
// the fine smoother, the lambda_max product), R is built in the pass that sums Hc, one GPU, the iterative solve.  Terms
// added to H after the fused launch and per-element materials are ruled out by mf.valid (claim_records).
static bool setup_records_eligible(tlfea_newton_t s) {
  if (setup_records_env() == 0 || (setup_records_env() < 0 && s->N < kFineMatfreeMinRows)) return false;
  if (s->lin.method != 0 || s->spmv32_every >= 2 || !lmax_matfree_env() || s->trace) return false;
  if (!matfree_chosen(s) || !fine_matfree_possible(s)) return false;
  const auto& m = s->pmg;
  return m.ok && pmg_rop_on(s) && m.rows.ok && m.rop.stream_cap > 0;
}
int tlfea::setup_records_decide(tlfea_newton_t s, bool* on) {
  *on = false;
  if (setup_records_env() == 0 || (setup_records_env() < 0 && s->N < kFineMatfreeMinRows)) return 0;
  if (!matfree_chosen(s) || !fine_matfree_possible(s)) return 0;
  TRY(pmg_prepare(s));
  if (!setup_records_eligible(s)) return 0;
  TRY(matfree_ensure_buffer(s));
  if (!s->mf.compact) return 0;
  TRY(setup_records_prepare(s));
  *on = s->sr.ok;
  return 0;
}
bool tlfea::setup_records_live(tlfea_newton_t s) {
  const auto& r = s->sr;
  return !r.h_current && r.ok && s->mf.valid && r.gen == s->mf.gen && setup_records_eligible(s) && s->mf.compact;
}
// In H's place: the image rows of R (with the pinned children's penalties) and the fine block diagonal d_D, from the
// records the assembly has just claimed.  The packed fp64 records are the CG product's: packed here, once per assembly.
int tlfea::setup_records_assemble(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  auto& r = s->sr;
  const auto& f = s->mf;
  const auto& ro = s->pmg.rop;
  TRY(matfree_ensure_records(s));
  launch_assemble_image(s->stream, d->view(), d->mat, s->prm.time_step, r.rg, s->av, s->d_Fq, r.d_cmass4,
                        d->mass_rho0 > 0.0 ? d->mass_rho0 : 0.0, r.d_img);
  launch_image_pinned(s->stream, r.n_ch, ro.d_ch, ro.d_ch_w, r.d_ch_row, r.d_ch_pos, ro.d_off, d->d_off, f.fixed, s->d_nw,
                      f.penalty, r.d_img);
  launch_records_diag(s->stream, d->view(), matfree_points(false), f.d_gp, f.d_Fp, f.mc, s->N, d->inc(), f.fixed, s->d_nw,
                      f.penalty, r.d_dbuf, s->d_D);
  r.gen = f.gen;
  HIP_TRY(hipGetLastError());
  return 0;
}

// Galerkin operators of the current H: Hc = P^T H P, H3 = P2^T Hc P2
// The one place that picks the kernel.  T10 with the row lists (pmg_prepare: a property of the mesh): the row kernel --
// with_R in the same pass as the streamed build of R (a matrix-free set-up), else alone; ANCF and meshes whose lists do
// not fit: the gather.  setup: the call of a preconditioner set-up, which wants the diagonal blocks in vertex.d_D too;
// returns whether they were written (the read-backs leave d_D alone).
// image: the rows of sr.d_img, assembled from the element records, stand in for the children's rows of H -- the same
// kernels through a second set of tables, one child of weight 1 per row whose "fine row" is the image row itself
// (hc_form 4; a set-up with R only).
static bool vertex_galerkin(tlfea_newton_t s, bool setup = false, bool with_R = false, bool image = false) {
  auto& m = s->pmg;
  if (image) {
    const auto& r = m.rop;
    const auto& g = m.rows;
    const auto& q = s->sr;
    PmgRows a;
    a.r_off = r.d_off; a.r_cols = r.d_cols; a.pos_off = r.d_off; a.con_pos = q.d_id_pos;
    a.ch_off = q.d_id_off; a.ch = q.d_id_ch; a.ch_w = q.d_id_w; a.f_off = r.d_off; a.Hval = q.d_img;
    a.g_row = g.d_row; a.g_off = g.d_off; a.g_pos = g.d_pos; a.g_w = g.d_w;
    a.c_off = m.vertex.d_off; a.c_upper = m.d_c_upper; a.c_mirror = m.d_c_mirror; a.cblk_row = m.d_cblk_row;
    a.Hc = m.vertex.d_H; a.D = m.vertex.d_D;
    a.sc_f = s->d_sc; a.R8 = r.d_R8; a.R1 = r.d_R1;
    launch_pmg_galerkin_rows(s->stream, m.vertex.N, g.cap, a, true, g.d_long_rows, g.n_long, g.ws_stride, g.ws_rows, g.d_ws);
    m.hc_form = 4;
    return true;
  }
  if (!m.rows.ok) {
    launch_pmg_galerkin(s->stream, m.n_upper, m.d_c_upper, m.d_c_mirror, m.vertex.d_off, m.d_cblk_row, m.d_con_off,
                        m.d_con_base, m.d_con_deg, m.d_con_w, s->d_H, m.vertex.d_H);
    m.hc_form = setup ? 1 : 0;
    return false;
  }
  const auto& r = m.rop;
  const auto& g = m.rows;
  PmgRows a;
  a.r_off = r.d_off; a.r_cols = r.d_cols; a.pos_off = r.d_pos_off; a.con_pos = r.d_con_pos;
  a.ch_off = r.d_ch_off; a.ch = r.d_ch; a.ch_w = r.d_ch_w; a.f_off = s->d->d_off; a.Hval = s->d_H;
  a.g_row = g.d_row; a.g_off = g.d_off; a.g_pos = g.d_pos; a.g_w = g.d_w;
  a.c_off = m.vertex.d_off; a.c_upper = m.d_c_upper; a.c_mirror = m.d_c_mirror; a.cblk_row = m.d_cblk_row;
  a.Hc = m.vertex.d_H; a.D = setup ? m.vertex.d_D : nullptr;
  a.sc_f = with_R ? s->d_sc : nullptr; a.R8 = with_R ? r.d_R8 : nullptr; a.R1 = with_R ? r.d_R1 : nullptr;
  launch_pmg_galerkin_rows(s->stream, m.vertex.N, g.cap, a, with_R, g.d_long_rows, g.n_long, g.ws_stride, g.ws_rows, g.d_ws);
  m.hc_form = !setup ? 0 : (with_R ? 3 : 2);
  return setup;
}
static void level3_galerkin(tlfea_newton_t s) {
  auto& g = s->pmg.agg;
  launch_agg_galerkin(s->stream, g.n_pairs, g.d_pair_A, g.d_pair_pos, g.d_pair_B, g.d_pcon_off, g.d_pcon_base, g.d_pcon_deg,
                      g.d_pcon_i, g.d_pcon_j, g.d_rvec, g.d_active, g.lvl.d_off, s->pmg.vertex.d_H, g.lvl.d_H);
}

// block-Jacobi scaling and low-precision copy of a coarse level whose d_H and d_D are current
static void level_scale_convert(tlfea_newton_t s, PolyLevel& L, int bits) {
  launch_invert_diag(s->stream, L.N, L.d_D, L.d_Dinv);
  launch_lp_scale(s->stream, L.N, L.d_D, L.d_Dinv, L.d_sc, L.d_Dinv_s);
  launch_lp_convert(s->stream, L.N, L.inc(), L.d_H, L.d_sc, nullptr, L.d_D, L.d_B8, L.d_B1, bits);
  launch_to_float(s->stream, (size_t)9 * L.N, L.d_Dinv_s, L.d_f32 + (size_t)18 * L.N);
}

// per solve, after H and the fine block diagonal are current: Hc = P^T H P, its block-Jacobi scaling and fp16 copy
static int pmg_build_level(tlfea_newton_t s) {
  auto& m = s->pmg;
  PolyLevel& V = m.vertex;
  const int bits = cheb_bits_eff(s);
  // The choice of the fine smoother comes first (it needs nothing computed below): where it falls on the matrix-free form
  // and R is built streamed, the pass that sums Hc builds R too, scaled with sc_c formed from the diagonal blocks it sums --
  // the bits the lp_scale launch below writes to V.d_sc from V.d_D (one GPU: no interface sum touches V.d_D in between).
  m.rop.built = false;
  const bool rop = pmg_rop_on(s);
  if (rop) {
    m.rop.built = true;
    TRY(fine_matfree_choose(s));
  }
  const bool fused = rop && s->fmf.now && m.rop.stream_cap > 0;
  // H was left unassembled (DESIGN 3g'): the fused pass runs on the image rows; a set-up that does not take the matrix-free
  // smoother and the streamed build of R after all gets H now and finishes on the CSR path
  const bool image = fused && setup_records_live(s);
  if (!image) TRY(hessian_current(s));
  s->sr.last_form = image ? 1 : 0;
  TRY(V.ensure_copy(bits));
  if (!vertex_galerkin(s, true, fused, image)) launch_extract_diag(s->stream, V.N, V.inc(), V.d_H, V.d_D);
  // multi-GPU: Hc = sum over ranks of P^T H_r P -- the diagonal blocks of boundary vertices are partial per rank
  if (s->ar) TRY(iface_sum_lvl(s, m.iface(), V.d_D, 9));
  // overlapping partition: rows of the outermost ghost layer are incomplete -- their diagonal blocks (hence the scaling of
  // their COLUMNS in every complete row) come from their owners
  TRY(halo_refresh_f64(s, 1, s->halo.depth, 9, V.d_D));
  level_scale_convert(s, V, bits);
  if (rop && !fused) {  // R = S_c P^T S_f^-1 Hs from the fine copy as stored (converted before it is read) and both scalings
    auto& r = m.rop;
    if (!s->fmf.now) TRY(ensure_fine_copy(s));  // a set-up that deferred the copy and does not take the form after all
    // where the fine smoother applies H itself (DESIGN 3g'), R from H's fp64 rows, so that both see one operator
    if (s->fmf.now)
      launch_pmg_rop_build_h(s->stream, V.N, r.d_off, r.d_cols, r.d_con_off, r.d_con_blk, r.d_con_ord, r.d_ch_off, r.d_ch,
                             r.d_ch_w, s->d->d_off, s->d_H, s->d_sc, V.d_sc, r.d_R8, r.d_R1);
    else
      launch_pmg_rop_build(s->stream, V.N, r.d_off, r.d_con_off, r.d_con_blk, r.d_con_ord, r.d_ch_off, r.d_ch, r.d_ch_w,
                           s->d_B8, s->d_B1, fine_bits(s), s->d_sc, V.d_sc, r.d_R8, r.d_R1);
  }
  if (m.agg.ok) {  // third level: H3 = P2^T Hc P2, its scaling and low-precision copy
    PolyLevel& A = m.agg.lvl;
    level3_galerkin(s);
    // overlapping partition: every rank summed the vertex-level rows it OWNS; the level is replicated, so the shares are
    // added once per Newton iteration (identical bits on every rank afterwards: the level-3 polynomial needs no exchange)
    if (s->halo.on) TRY(call_allreduce(s, A.d_H, 9 * A.nnz));
    TRY(A.ensure_copy(bits));
    launch_extract_diag(s->stream, A.N, A.inc(), A.d_H, A.d_D);
    level_scale_convert(s, A, bits);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// lambda_max(D^-1 H) of a coarse level by power iteration on its first `rows` rows, warm-started from the vector the level
// keeps: 16 products from the scaling vector (positive on every DOF) when cold, 2 when warm.
// iface given: the level follows the partition (vertex level).  Norms weigh replicated DOFs by w and are summed over ranks,
//   ghost layer 1 of the vector is refreshed before and the boundary rows of H v are summed after every product: every
//   rank ends with the same estimate.  iface null: the level is replicated (third level), no exchange of any kind.
static int level_lam_max(tlfea_newton_t s, PolyLevel& L, int rows, const double* w, const LevelIface* iface,
                         const char* name) {
  const int n = 3 * rows;
  const bool cold = !(L.lam > 0.0);
  if (cold)
    HIP_TRY(hipMemcpyAsync(L.d_eigv, L.d_sc, 3 * (size_t)L.N * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  auto normalise = [&]() -> int {  // v <- v / ||v||, the norm stays on the device
    if (iface)
      TRY(device_sumsq_async(s, L.d_eigv, w, n));
    else
      launch_norm2(s->stream, L.d_eigv, nullptr, n, part(s, 5), s->d_scal);
    launch_scale_inv_sqrt(s->stream, n, s->d_scal, L.d_eigv);
    return 0;
  };
  TRY(normalise());
  for (int k = 0; k < (cold ? 16 : 2); k++) {
    if (iface) TRY(halo_refresh_f64(s, 1, 1, 3, L.d_eigv));
    launch_spmv_dir_dot(s->stream, rows, L.inc(), L.d_H, L.d_eigv, L.d_eigv, 1, part(s, 1), part(s, 0), L.d_p, L.d_q,
                        part(s, 2), false, false);
    if (iface) TRY(iface_sum_lvl(s, *iface, L.d_q, 3));
    launch_apply_dinv(s->stream, rows, L.d_Dinv, L.d_q, L.d_eigv);
    TRY(normalise());
  }
  double ss = 0.0;
  TRY(fetch_scalar(s, s->d_scal, &ss));
  if (!(ss > 0.0)) return fail(std::string("p-multigrid: ") + name + " lambda_max estimate failed");
  L.lam = std::sqrt(ss);
  return 0;
}

// lambda_max of the coarse levels, then the cycle's coefficient table (pmg_coef.h) to the device
int tlfea::pmg_coefficients(tlfea_newton_t s) {
  auto& m = s->pmg;
  const LevelIface ic = m.iface();
  // overlapping partition: the vertex level's iteration lives on the owned rows
  TRY(level_lam_max(s, m.vertex, s->halo.on ? s->halo.rows_c(0) : m.vertex.N, dist_on(s) ? m.d_wc3 : nullptr, &ic, "coarse"));
  if (m.agg.ok) TRY(level_lam_max(s, m.agg.lvl, m.agg.lvl.N, nullptr, nullptr, "level-3"));
  const PmgTable t = pmg_table(s);
  const bool l3 = t.levels == 3;  // the vertex level smooths like the fine one, the polynomial solve moves to level 3
  const PmgInterval fine{s->lam_safety * s->lam_max, pmg_kappa_s(s)};
  const PmgInterval vertex{s->lam_safety * m.vertex.lam, l3 ? pmg_kappa_s2(s) : pmg_kappa_coarse(t.kc)};
  const PmgInterval level3 = l3 ? PmgInterval{s->lam_safety * m.agg.lvl.lam, pmg_kappa_level3(t.k3)} : PmgInterval();
  double* h = s->h_pin + 8;
  pmg_table_fill(t, pmg_smoother_kind(), fine, vertex, level3, h);
  HIP_TRY(hipMemcpyAsync(m.d_coef, h, (size_t)t.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
  return 0;
}

// One step of a partitioned level's polynomial (tlfea_newton_set_interface): this rank's partial boundary rows of Hs d ->
// all-reduce -> the fused step reads the sums.  One collective per step.  w: weights of the r.z partials (last step).
static int c32_step_iface(tlfea_newton_t s, const C32Level& L, const LevelIface& I, C32Vecs& v, int rows, const double* coef,
                          const double* d_r, double* d_z, double* rz_part, bool last, const double* w) {
  const int nb = 3 * I.n_glob;
  if (nb) HIP_TRY(hipMemsetAsync(s->d_ibuf, 0, (size_t)nb * sizeof(double), s->stream));
  launch_spmv32_rows(s->stream, I.n_loc, I.d_node, I.d_slot, L.inc, L.B8, L.B1, L.bits, v.d, s->d_ibuf);
  if (nb) TRY(call_allreduce(s, s->d_ibuf, nb));
  c32_step(s, L, v, rows, coef, d_r, d_z, rz_part, last, C32Bnd{I.d_bslot, s->d_ibuf, w});
  return 0;
}

// z = V-cycle(r); the last fine step leaves the r.z slots in rz_part.  init_done: the previous iteration's update
// kernel already wrote the fine start vectors.
static int pmg_apply(tlfea_newton_t s, const double* d_r, double* d_z, double* rz_part, bool init_done) {
  auto& m = s->pmg;
  const PolyLevel& V = m.vertex;
  const int N = s->N, Nc = V.N, bits = cheb_bits_eff(s);
  const PmgTable t = pmg_table(s);
  const int ks = t.ks;
  const double* cf = m.d_coef;
  const double* cc = cf + t.coarse();  // the vertex level's pairs
  if (!s->fmf.now) TRY(ensure_fine_copy(s));  // the fine passes stream the stored copy (before fine_c32 takes its pointers)
  const C32Level Lf = fine_c32(s), Lc = V.c32(bits, 1);
  C32Vecs f(s->d_f32, 3 * (size_t)N), c(V.d_f32, 3 * (size_t)Nc);
  if (s->ar) {
    // Multi-GPU V-cycle: the same sequence, every polynomial step on either level preceded by the exchange of the
    // partition-boundary rows of Hs d, the restriction by the exchange of the boundary vertices' restricted residuals.
    // One collective per step: 2 ks on the fine level, kc - 1 on the coarse level, 1 for the restriction.
    if (m.agg.ok) return fail("p-multigrid: the third level is single-GPU only");
    const LevelIface If = s->iface(), Ic = m.iface();
    auto fine = [&](const double* co, bool last) {
      return c32_step_iface(s, Lf, If, f, N, co, d_r, d_z, rz_part, last, s->d_w);
    };
    launch_cheb32_init(s->stream, N, f.Dinv_f, d_r, s->d_sc, cf, f.d, f.z, f.r);
    for (int k = 1; k < ks; k++) TRY(fine(cf + 2 * k, false));
    TRY(fine(cf + t.resid(), false));
    const int nb = 3 * Ic.n_glob;
    if (nb) HIP_TRY(hipMemsetAsync(s->d_ibuf, 0, (size_t)nb * sizeof(double), s->stream));
    launch_pmg_restrict_rows(s->stream, Ic.n_loc, Ic.d_node, Ic.d_slot, m.d_child_off, m.d_child, m.d_child_w_dist, f.r,
                             s->d_sc, s->d_ibuf);
    if (nb) TRY(call_allreduce(s, s->d_ibuf, nb));
    launch_pmg_restrict_init(s->stream, Nc, m.d_child_off, m.d_child, m.d_child_w, f.r, s->d_sc, V.d_sc, c.Dinv_f, cc, c.d, c.z,
                             c.r, Ic.d_bslot, s->d_ibuf);
    for (int k = 1; k < t.kc; k++) TRY(c32_step_iface(s, Lc, Ic, c, Nc, cc + 2 * k, d_r, d_z, rz_part, false, nullptr));
    launch_pmg_prolong(s->stream, N, m.d_par0, m.d_par1, c.z, V.d_sc, s->d_sc, f.z, f.d);
    TRY(fine(cf + t.restart(), ks == 1));
    for (int k = 1; k < ks; k++) TRY(fine(cf + 2 * k, k == ks - 1));
    return 0;
  }
  // pre-smooth: d0 = (SDS)^-1 r^/theta ; ks - 1 Chebyshev steps ; residual of the result (coefficients (0,0): res -= Hs d)
  // Overlapping partition: r comes in exact on layers <= halo_dr(); every fine pass gives up one layer (the restriction
  // needs layer 1 after the ks pre-smoothing passes, the post-smoother's pointwise operands layer ks - 1), so the fine
  // launches stop at that row count -- deeper ghosts are never computed, they would only accumulate garbage -- and the
  // r.z slots weigh owned DOFs only.
  const bool hal = s->halo.on;
  const int Nf = hal ? s->halo.rows(halo_dr(s)) : N;
  const bool weighted = pmg_smoother_kind() != 1;  // fourth-kind smoother: z^ += beta_k d
  const double* betas = cf + t.beta();
  const C32Bnd bnd_f = hal ? C32Bnd{nullptr, nullptr, s->d_w} : C32Bnd();
  // from the element records where this set-up chose that form and the records still belong to the assembled H
  // (DESIGN 3g': two launches, the ping-pong partners swap as in c32_step), else the stream of the low-precision copy
  // R of this set-up came from H itself: streaming the fp16 copy now would smooth and restrict with two operators
  if (s->fmf.now && !fine_matfree_live(s))
    return fail("p-multigrid: the element records no longer belong to the H this preconditioner was set up for (a residual "
                "evaluation or an assembly since the set-up); set the preconditioner up again");
  const bool fmf = s->fmf.now;
  auto fine = [&](const double* co, bool last, const double* zw) {  // one fine pass
    if (fmf) {
      launch_fine_matfree_apply(s->stream, s->d->view(), s->fmf.v, f.d, s->mf.cp);
      launch_fine_matfree_step(s->stream, N, s->fmf.v, s->mf.cp, f.Dinv_f, s->d_sc, f.d, co, weighted ? zw : nullptr, f.d2, f.z,
                               f.z2, f.r, f.r2, d_r, d_z, rz_part, last);
      f.swap();
      return;
    }
    C32Bnd bnd = bnd_f;
    bnd.zw = weighted ? zw : nullptr;
    c32_step(s, Lf, f, Nf, co, d_r, d_z, rz_part, last, bnd);
  };
  if (!init_done) launch_cheb32_init(s->stream, Nf, f.Dinv_f, d_r, s->d_sc, cf, f.d, f.z, f.r);
  for (int k = 1; k < ks; k++) fine(cf + 2 * k, false, betas + k);
  // Restriction through the stored operator (pmg_rop_on): the residual pass is dropped.  f.r is res_A = r^ - Hs (z^ - d_last)
  // and f.d the last direction; the residual is linear in the direction, so the coarse right-hand side is
  // S_c P^T S_f^-1 res_A - R d_last, the prolongation writes d := d_last + corr, and the restart pass below forms
  // res_A - Hs (d_last + corr) -- what the residual pass and the restart pass formed together.
  const bool rop = pmg_rop_now(s);
  if (rop) {
    launch_pmg_restrict_op_init(s->stream, Nc, m.rop.nnz, m.d_child_off, m.d_child, m.d_child_w, f.r, f.d, s->d_sc, V.d_sc,
                                m.rop.d_off, m.rop.d_cols, m.rop.d_R8, m.rop.d_R1, c.Dinv_f, cc, c.d, c.z, c.r);
  } else if (weighted) {
    // Weighted z^ updates: the residual the recurrence carries is the UNWEIGHTED iterate's, not that of z^ -- restricting it
    // made the cycle unsymmetric (defect 3e-4 on res2; tests/test_gpu_precond_operator.py, configuration 11).  Form
    // res^ = S r - Hs z^ itself: start vectors into the spare buffers (res^ := S r), then one pass with z^ as the direction
    // and the pair (0, 0), which leaves z^ as it is.  Not a c32_step: it reads z^ as the direction, writes into the spare
    // buffers and swaps z^ only.
    launch_cheb32_init(s->stream, Nf, f.Dinv_f, d_r, s->d_sc, cf, f.d2, f.z2, f.r2);
    launch_cheb32(s->stream, Nf, Lf.nnz, Lf.inc, Lf.B8, Lf.B1, Lf.bits, f.Dinv_f, Lf.sc, f.z, cf + t.resid(), f.d2, f.z, f.z2,
                  f.r2, f.r, d_r, d_z, rz_part, false, bnd_f, s->geo_out(0, false));
    std::swap(f.z, f.z2);
  } else
    fine(cf + t.resid(), false, nullptr);
  // coarse correction
  if (!rop)
    launch_pmg_restrict_init(s->stream, Nc, m.d_child_off, m.d_child, m.d_child_w, f.r, s->d_sc, V.d_sc, c.Dinv_f, cc, c.d, c.z,
                             c.r);
  // Overlapping partition: the restricted residual is exact on the owned vertices only.  A refresh makes the three
  // vectors exact on every ghost layer (G of them).  Rows of Hc are exact up to layer G - 2 (a vertex of layer G - 1 has
  // mid-edge children in the outermost fine layer, whose rows of H are incomplete), so the first step after a refresh
  // leaves layers <= G - 2 exact and every further step gives up one more; the prolongation needs ks + 1 layers at the
  // end (ks fine passes follow).  One exchange buys up to G - 1 steps, computed redundantly on the overlap.
  const int G = s->halo.depth, need_end = ks + 1;
  int valid = 0;
  auto mid = [&](const double* co) -> int {  // one vertex-level pass
    if (hal && valid < 1) {
      TRY(halo_refresh_f32(s, 1, G, 3, c.d, c.z, c.r));
      valid = G - 1;
    }
    c32_step(s, Lc, c, Nc, co, d_r, d_z, rz_part, false);
    valid--;
    return 0;
  };
  if (m.agg.ok) {
    // vertex level as a smoothing level: the fine level's sequence once more, with the level-3 polynomial inside.
    // Overlapping partition: the third level is REPLICATED -- its residual is summed over the ranks' owned members (one
    // small all-reduce), its polynomial runs redundantly with no exchange, and its correction is exact on every vertex a
    // rank holds (so it does not touch the validity count).
    auto& g = m.agg;
    const PolyLevel& A = g.lvl;
    const C32Level L3 = A.c32(bits, 2);
    C32Vecs a(A.d_f32, 3 * (size_t)A.N);
    const double* c3 = cf + t.level3();
    for (int k = 1; k < t.ks2; k++) TRY(mid(cc + 2 * k));  // Chebyshev steps of the pre-smoother
    TRY(mid(cf + t.coarse_resid()));                       // (0,0): residual of the result
    if (hal) {
      launch_agg_restrict(s->stream, A.N, g.d_mem_off, g.d_mem, g.d_rvec, c.r, V.d_sc, g.d_r3);
      TRY(call_allreduce(s, g.d_r3, 3 * A.N));
      launch_agg_init3(s->stream, A.N, g.d_r3, A.d_sc, a.Dinv_f, c3, a.d, a.z, a.r);
    } else
      launch_agg_restrict_init(s->stream, A.N, g.d_mem_off, g.d_mem, g.d_rvec, c.r, V.d_sc, A.d_sc, a.Dinv_f, c3, a.d, a.z, a.r);
    for (int k = 1; k < t.k3; k++) c32_step(s, L3, a, A.N, c3 + 2 * k, d_r, d_z, rz_part, false);
    launch_agg_prolong(s->stream, Nc, g.d_agg, g.d_rvec, a.z, A.d_sc, V.d_sc, c.z, c.d);  // z^ += corr ; d := corr
    TRY(mid(cf + t.coarse_restart()));                     // (0, 1/theta): res^ -= Hs corr, restart
    for (int k = 1; k < t.ks2; k++) TRY(mid(cc + 2 * k));  // the remaining terms; the vertex-level result is in c.z
  } else
    for (int k = 1; k < t.kc; k++) TRY(mid(cc + 2 * k));
  if (hal && valid < need_end) TRY(halo_refresh_f32(s, 1, need_end, 3, c.z));  // the last chunk ended too shallow
  // z^ += corr ; d := corr (restricted operator: d := d_last + corr)
  launch_pmg_prolong(s->stream, Nf, m.d_par0, m.d_par1, c.z, V.d_sc, s->d_sc, f.z, f.d, rop);
  // post-smooth: res^ -= Hs corr ; d0' = (SDS)^-1 res^/theta ; z^ += d0'   == one step with coefficients (0, 1/theta),
  // then the ks - 1 Chebyshev steps that complete the polynomial; the last pass returns z = S z^ (fp64) and the r.z slots
  fine(cf + t.restart(), ks == 1, betas);
  for (int k = 1; k < ks; k++) fine(cf + 2 * k, k == ks - 1, betas + k);
  return 0;
}

// z = M^-1 r with the preconditioner precond_setup() prepared: the p-multigrid cycle, the Chebyshev polynomial (12 x 12
// node blocks on the ANCF kinds: z = L^-T p(L^-1 H L^-T) L^-1 r, the polynomial's r.z slots are r^.z^ = r.z) or the inverse
// 3 x 3 diagonal blocks.  The one function behind a CG iteration of pcg(), the modal solve and the test hook
// tlfea_newton_apply_preconditioner; the last fine step leaves the r.z slots in rz_part.  init_done: the previous CG
// iteration's update kernel already wrote the fp32 start vectors.
int tlfea::precond_apply(tlfea_newton_t s, const double* d_r, double* d_z, double* rz_part, bool init_done) {
  if (cheb_degree_eff(s) <= 1) {
    launch_apply_dinv(s->stream, s->N, s->d_Dinv, d_r, d_z);
    return 0;
  }
  if (precond_eff(s) == 2) return pmg_apply(s, d_r, d_z, rz_part, init_done);
  if (blk12_now(s)) {
    launch_blk12_apply(s->stream, s->N / 4, s->d_L12inv_f, false, d_r, s->d_cd);
    TRY(cheb_apply(s, s->d_cd, s->d_cd2, rz_part, false));
    launch_blk12_apply(s->stream, s->N / 4, s->d_L12inv_f, true, s->d_cd2, d_z);
    return 0;
  }
  return cheb_apply(s, d_r, d_z, rz_part, init_done);
}

// What the preconditioner needs from the current H, in the launches and the order pcg() has always issued them.
// Stage 0, before the start residual: the block diagonal, its inverse and the scaled low-precision copy.  Stage 1, after
// it (d_b: start vector of a cold lambda_max estimate): lambda_max, the polynomial's coefficients and the p-multigrid
// levels.  pcg() runs its start residual between the two; the modal solve calls them back to back.
int tlfea::precond_setup(tlfea_newton_t s, const double* d_b, int stage) {
  tlfea_t10_t d = s->d;
  const int N = s->N;
  if (stage == 0) {
    TRY(refuse_empty_rows(s, "preconditioner set-up"));  // extract_dinv_kernel / extract_diag read every row's diagonal block
    const bool lp = cheb_bits_eff(s) != 64;
    s->lp_scaled = s->lp_current = false;  // the stored copy belonged to the last set-up's H
    // H left unassembled by the Newton loop (DESIGN 3g'): d_D is already the block diagonal of the records' H
    // (setup_records_assemble); a set-up that can no longer run from the records gets H first
    const bool rec = lp && setup_records_live(s);
    if (!rec) TRY(hessian_current(s));
    s->sr.last_form = 0;
    if (s->ar || lp) {
      // diagonal blocks of partition-boundary nodes are partial per rank: sum them before inverting
      if (!rec) launch_extract_diag(s->stream, N, d->inc(), s->d_H, s->d_D);
      TRY(iface_sum(s, s->d_D, 9));
      // overlapping partition: the outermost ghost layer's rows are incomplete -- its diagonal blocks (the scaling of its
      // columns in every complete row) come from their owners
      TRY(halo_refresh_f64(s, 0, s->halo.depth, 9, s->d_D));
      launch_invert_diag(s->stream, N, s->d_D, s->d_Dinv);
      // The copy waits where stage 1 can still choose the fine smoother from the element records (only R having been
      // built is open); every other configuration converts here, in the launch order it always had.  The mixed-precision
      // iteration, which pcg() switches on after this stage, rules the form out.
      if (lp) TRY(lp_build(s, fine_matfree_possible(s) && s->spmv32_every < 2));
    } else {
      launch_extract_dinv(s->stream, N, d->inc(), s->d_H, s->d_Dinv);
    }
    return 0;
  }
  s->fmf.now = false;
  s->fmf.last = 0;
  if (cheb_degree_eff(s) > 1) {
    TRY(estimate_lam_max(s, d_b));
    TRY(cheb_upload_coefficients(s));
    if (precond_eff(s) == 2) {
      TRY(pmg_prepare(s));
      if (precond_eff(s) == 2) {  // still available after the set-up attempt
        TRY(pmg_build_level(s));
        TRY(pmg_coefficients(s));
        TRY(fine_matfree_setup(s));  // the fine smoother's form for this set-up (DESIGN 3g')
      }
    }
  }
  // a deferred copy whose set-up never reached the choice (no hierarchy for this mesh, no R): everything but the form reads it
  if (!s->fmf.now) TRY(ensure_fine_copy(s));
  return 0;
}

// The set-up of a call that runs no start residual between the stages (modal solve, the operator hook): both stages, then
// the flag of the node-block factorisation once the stream is drained.  Stage 1 runs on the factors stage 0 left: where
// a block was not positive definite they are not those of H, and the lambda_max estimate on them can fail first (NaN) -- the
// flag names the cause, so it is read before a failure of stage 1 is reported.
int tlfea::precond_setup_whole(tlfea_newton_t s, const double* d_b, const char* who) {
  TRY(precond_setup(s, d_b, 0));
  const int rc1 = precond_setup(s, d_b, 1);
  const std::string why1 = rc1 ? api_error() : std::string();
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (cheb_bits_eff(s) != 64 && blk12_now(s)) {
    int bad = 0;
    HIP_TRY(hipMemcpy(&bad, s->d_blk12_err, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return fail(std::string(who) + ": a 12 x 12 node block of H is not positive definite (H is not SPD)");
  }
  if (rc1) api_error() = why1;
  return rc1;
}

// Test hooks of the p-multigrid level: sizes, then the parent map and the Galerkin operator Hc = P^T H P of the CURRENT H
// in the same DOF-level layout as H (rows 3 Nc, node row -> [d][k][e]); builds the hierarchy if needed.
extern "C" int tlfea_newton_pmg_sizes(tlfea_newton_t s, int* n_coarse, int* nnz_coarse_blocks) {
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  TRY(pmg_prepare(s));
  if (!s->pmg.ok) return fail("p-multigrid is not available for this mesh");
  *n_coarse = s->pmg.vertex.N;
  *nnz_coarse_blocks = s->pmg.vertex.nnz;
  return 0;
}
extern "C" int tlfea_newton_pmg_retrieve(tlfea_newton_t s, int* par0, int* par1, int* c_off, int* c_cols, double* Hc) {
  int nc = 0, nnz = 0;
  TRY(tlfea_newton_pmg_sizes(s, &nc, &nnz));
  auto& m = s->pmg;
  TRY(hessian_current(s));
  vertex_galerkin(s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  D2H(par0, m.d_par0, (size_t)s->N);
  D2H(par1, m.d_par1, (size_t)s->N);
  D2H(c_off, m.vertex.d_off, (size_t)nc + 1);
  D2H(c_cols, m.vertex.d_cols, (size_t)nnz);
  D2H(Hc, m.vertex.d_H, (size_t)9 * nnz);
  return 0;
}
// Hc as the LAST preconditioner set-up left it on the device, nothing recomputed (tlfea_newton_pmg_retrieve and
// tlfea_newton_pmg3_retrieve sum it again, on their own): the values, and which kernel summed them -- 1 the gather over the
// contribution lists, 2 the row kernel alone, 3 the row kernel fused with the build of R
extern "C" int tlfea_newton_pmg_retrieve_built(tlfea_newton_t s, double* Hc, int* form) {
  if (!s || !Hc || !form) return fail("tlfea_newton_pmg_retrieve_built: null argument");
  const auto& m = s->pmg;
  if (!m.ok || !m.hc_form || !m.vertex.d_H)
    return fail("tlfea_newton_pmg_retrieve_built: no p-multigrid set-up has left Hc on this solver since the last read-back that "
                "recomputes it");
  HIP_TRY(hipStreamSynchronize(s->stream));
  D2H(Hc, m.vertex.d_H, (size_t)9 * m.vertex.nnz);
  *form = m.hc_form;
  return 0;
}
// the fine block diagonal [N][9] as the last stage-0 set-up (or the last assembly from the element records) left it
extern "C" int tlfea_newton_get_block_diagonal(tlfea_newton_t s, double* D) {
  if (!s || !D) return fail("tlfea_newton_get_block_diagonal: null argument");
  if (!s->d_D) return fail("tlfea_newton_get_block_diagonal: this solver keeps no block diagonal (no low-precision set-up)");
  HIP_TRY(hipStreamSynchronize(s->stream));
  D2H(D, s->d_D, (size_t)9 * s->N);
  return 0;
}
// the image rows of R as the last assembly from the element records left them (DESIGN 3g'), nothing recomputed
extern "C" int tlfea_newton_get_setup_image(tlfea_newton_t s, double* image, long long* len) {
  if (!s || !len) return fail("tlfea_newton_get_setup_image: null argument");
  const auto& r = s->sr;
  if (!r.ok || !r.d_img || r.gen < 0)
    return fail("tlfea_newton_get_setup_image: no Newton iteration of this solver has been set up from the element records");
  *len = (long long)9 * s->pmg.rop.nnz;
  if (image) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    D2H(image, r.d_img, (size_t)9 * s->pmg.rop.nnz);
  }
  return 0;
}

// Test hooks of the restricted fine operator: what the LAST preconditioner set-up (a solve or
// tlfea_newton_apply_preconditioner) left on the device, nothing is rebuilt.  Sizes; R as stored (values widened to
// double, [nnz][9] row-major per block); the fine level's stored copy in the node-block CSR of H, widened likewise,
// with both scalings.
// Read-back of the polynomial step's launch geometry (c32_geometry.h): regime (0 last, 1 bandwidth, 2 latency, 3 one-round;
// -1: no such launch yet), lanes per row, threads per workgroup, blocks per lane issued up front, rows per group, grid of
// the last NON-FINAL step launched on level 0 (fine), 1 (vertex) or 2 (third level) by a solve or the preconditioner hook,
// and the occupancy query's answer for the instantiation launched.  Recorded where the host issues the launch: a captured
// CG graph records it at capture, its replays do not touch it.
extern "C" int tlfea_newton_get_c32_geometry(tlfea_newton_t s, int level, int* out7) {
  if (!s || !out7) return fail("tlfea_newton_get_c32_geometry: null argument");
  if (level < 0 || level > 2) return fail("tlfea_newton_get_c32_geometry: level must be 0, 1 or 2");
  const C32Geometry& g = s->c32_geo[level];
  out7[0] = g.regime;
  out7[1] = g.lanes;
  out7[2] = g.threads;
  out7[3] = g.upfront;
  out7[4] = g.rows_per_group;
  out7[5] = g.grid;
  out7[6] = g.resident;
  return 0;
}
extern "C" int tlfea_newton_pmg_restrict_op_sizes(tlfea_newton_t s, int* out6) {
  if (!s || !out6) return fail("tlfea_newton_pmg_restrict_op_sizes: null argument");
  const auto& m = s->pmg;
  const bool have = m.ok && m.rop.ok && m.rop.built;
  out6[0] = have ? 1 : 0;
  out6[1] = m.ok ? m.vertex.N : 0;
  out6[2] = have ? m.rop.nnz : 0;
  out6[3] = have ? m.rop.n_con : 0;
  out6[4] = s->d->nnz_coef;
  out6[5] = s->d_B8 ? s->lp_bits_alloc : 0;
  return 0;
}
static int widen_to_host(tlfea_newton_t s, size_t nnz, const void* B8, const void* B1, int bits, double* out) {
  double* d_tmp = nullptr;
  TRY(dmalloc(&d_tmp, 9 * nnz));
  launch_lp_widen(s->stream, nnz, B8, B1, bits, d_tmp);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d_tmp, 9 * nnz * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d_tmp);
  HIP_TRY(e);
  return 0;
}
extern "C" int tlfea_newton_pmg_restrict_op_retrieve(tlfea_newton_t s, int* off, int* cols, double* vals) {
  if (!s || !off || !cols || !vals) return fail("tlfea_newton_pmg_restrict_op_retrieve: null argument");
  const auto& m = s->pmg;
  if (!(m.ok && m.rop.ok && m.rop.built))
    return fail("tlfea_newton_pmg_restrict_op_retrieve: the last preconditioner set-up built no restricted operator");
  HIP_TRY(hipStreamSynchronize(s->stream));
  D2H(off, m.rop.d_off, (size_t)m.vertex.N + 1);
  D2H(cols, m.rop.d_cols, (size_t)m.rop.nnz);
  return widen_to_host(s, (size_t)m.rop.nnz, m.rop.d_R8, m.rop.d_R1, 32, vals);
}
// Test hook: [0] bits of the fine copy allocated (0: none), [1] the copy is that of the last set-up's H, [2] fine-level
// conversions since creation
extern "C" int tlfea_newton_get_fine_copy_state(tlfea_newton_t s, int* out3) {
  if (!s || !out3) return fail("tlfea_newton_get_fine_copy_state: null argument");
  out3[0] = s->d_B8 ? s->lp_bits_alloc : 0;
  out3[1] = s->d_B8 && s->lp_current ? 1 : 0;
  out3[2] = s->lp_converts;
  return 0;
}
extern "C" int tlfea_newton_pmg_fine_copy_retrieve(tlfea_newton_t s, int* off, int* cols, double* vals, double* sc_f,
                                                   double* sc_c) {
  if (!s || !off || !cols || !vals || !sc_f || !sc_c) return fail("tlfea_newton_pmg_fine_copy_retrieve: null argument");
  const auto& m = s->pmg;
  TRY(ensure_fine_copy(s));  // a set-up that chose the matrix-free fine smoother left it unconverted
  const int bits = s->d_B8 ? s->lp_bits_alloc : 0;
  if (!m.ok || !m.vertex.d_sc || !s->d_sc || (bits != 16 && bits != 32))
    return fail("tlfea_newton_pmg_fine_copy_retrieve: no p-multigrid set-up with a 16- or 32-bit fine copy on the device");
  tlfea_t10_t d = s->d;
  HIP_TRY(hipStreamSynchronize(s->stream));
  std::copy(d->h_off.begin(), d->h_off.begin() + d->N + 1, off);
  std::copy(d->h_cols.begin(), d->h_cols.begin() + d->nnz_coef, cols);
  D2H(sc_f, s->d_sc, 3 * (size_t)s->N);
  D2H(sc_c, m.vertex.d_sc, 3 * (size_t)m.vertex.N);
  return widen_to_host(s, (size_t)d->nnz_coef, s->d_B8, s->d_B1, bits, vals);
}

// third level (opt-in, TLFEA_PMG_LEVELS=3): sizes, and everything
// needed to rebuild P2 and check H3 = P2^T Hc P2 on the host
extern "C" int tlfea_newton_pmg3_sizes(tlfea_newton_t s, int* n_aggregates, int* nnz_blocks, int* degree) {
  int nc = 0, nnz = 0;
  TRY(tlfea_newton_pmg_sizes(s, &nc, &nnz));
  const auto& g = s->pmg.agg;
  if (n_aggregates) *n_aggregates = g.ok ? g.Na : 0;
  if (nnz_blocks) *nnz_blocks = g.ok ? g.lvl.nnz : 0;
  if (degree) *degree = g.ok ? pmg_level3_degree(g.lvl.N) : 0;
  return 0;
}
extern "C" int tlfea_newton_pmg3_retrieve(tlfea_newton_t s, int* agg, double* rvec, int* active, int* off3, int* cols3,
                                          double* H3) {
  int nc = 0, nnz = 0;
  TRY(tlfea_newton_pmg_sizes(s, &nc, &nnz));
  auto& g = s->pmg.agg;
  if (!g.ok) return fail("p-multigrid: no third level on this mesh");
  TRY(hessian_current(s));
  vertex_galerkin(s);
  level3_galerkin(s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  D2H(agg, g.d_agg, (size_t)nc);
  D2H(rvec, g.d_rvec, (size_t)3 * nc);
  D2H(active, g.d_active, (size_t)g.Na);
  D2H(off3, g.lvl.d_off, (size_t)g.lvl.N + 1);
  D2H(cols3, g.lvl.d_cols, (size_t)g.lvl.nnz);
  D2H(H3, g.lvl.d_H, (size_t)9 * g.lvl.nnz);
  return 0;
}

// shape of the p-multigrid cycle a solve would run now: out6 = levels (0: none), fine smoother terms, vertex-level smoother
// terms (three levels) or 0, vertex-level polynomial degree (two levels) or 0, level-3 polynomial degree or 0, level-3 nodes
extern "C" int tlfea_newton_pmg_cycle_info(tlfea_newton_t s, int* out6) {
  if (!s || !out6) return fail("null argument");
  for (int k = 0; k < 6; k++) out6[k] = 0;
  if (precond_eff(s) != 2 || !s->pmg.ok) return 0;
  const PmgTable t = pmg_table(s);
  out6[0] = t.levels;
  out6[1] = t.ks;
  out6[2] = t.ks2;
  out6[3] = t.kc;
  out6[4] = t.k3;
  out6[5] = t.levels == 3 ? s->pmg.agg.lvl.N : 0;
  return 0;
}
extern "C" int tlfea_newton_polynomial_info(tlfea_newton_t s, int* out3) {
  if (!s || !out3) return fail("null argument");
  out3[0] = cheb_degree_eff(s);
  out3[1] = (int)std::lround(cheb_kappa_eff(s));
  out3[2] = blk12_now(s) ? 12 : 3;
  return 0;
}
extern "C" int tlfea_newton_pmg_coarse_degree(tlfea_newton_t s) { return s && s->pmg.ok ? pmg_coarse_degree_eff(s) : 0; }
extern "C" int tlfea_newton_get_precond(tlfea_newton_t s) {  // 1 Chebyshev polynomial, 2 p-multigrid (what a solve would use now)
  if (!s) return -1;
  return cheb_degree_eff(s) > 1 ? precond_eff(s) : 0;
}
// Test hook: ONE fine pass of the form of DESIGN 3g' (apply + gather-and-step) with the set-up a preceding
// tlfea_newton_apply_preconditioner left, on host vectors: d, res, z float [3N], r double [3N], the pair coef[2], zw (0:
// none), last.  Out: d', and either z^', res^' (float) or z = S z^' (double) and the kNPart r.z slots.
extern "C" int tlfea_newton_fine_smoother_pass(tlfea_newton_t s, const float* d, const float* res, const float* z, const double* r,
                                               const double* coef2, double zw, int last, float* d_out, float* z_out,
                                               float* res_out, double* z64_out, double* rz_slots) {
  if (!s || !d || !res || !z || !r || !coef2 || !d_out) return fail("tlfea_newton_fine_smoother_pass: null argument");
  if (!fine_matfree_live(s))
    return fail("tlfea_newton_fine_smoother_pass: the last preconditioner set-up did not choose the fine smoother from the "
                "element records, or the records have changed since");
  const int N = s->N;
  const size_t n = 3 * (size_t)N;
  C32Vecs f(s->d_f32, n);
  double* d_cf = nullptr;
  TRY(dmalloc(&d_cf, 3));
  const double cf[3] = {coef2[0], coef2[1], zw};
  auto run = [&]() -> int {
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(d_cf, cf, sizeof cf, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(f.d, d, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(f.r, res, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(f.z, z, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_r, r, n * sizeof(double), hipMemcpyHostToDevice));
    launch_fine_matfree_apply(s->stream, s->d->view(), s->fmf.v, f.d, s->mf.cp);
    launch_fine_matfree_step(s->stream, N, s->fmf.v, s->mf.cp, f.Dinv_f, s->d_sc, f.d, d_cf, zw != 0.0 ? d_cf + 2 : nullptr, f.d2,
                             f.z, f.z2, f.r, f.r2, s->d_r, s->d_zv, part(s, 0), last != 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(d_out, f.d2, n * sizeof(float), hipMemcpyDeviceToHost));
    if (last) {
      if (z64_out) HIP_TRY(hipMemcpy(z64_out, s->d_zv, n * sizeof(double), hipMemcpyDeviceToHost));
      if (rz_slots) HIP_TRY(hipMemcpy(rz_slots, part(s, 0), (size_t)kNPart * sizeof(double), hipMemcpyDeviceToHost));
    } else {
      if (z_out) HIP_TRY(hipMemcpy(z_out, f.z2, n * sizeof(float), hipMemcpyDeviceToHost));
      if (res_out) HIP_TRY(hipMemcpy(res_out, f.r2, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
  };
  const int rc = run();
  (void)hipFree(d_cf);
  return rc;
}
// fine smoother the last preconditioner set-up chose: 0 stream of the low-precision copy, 1 from the element records
extern "C" int tlfea_newton_get_fine_smoother(tlfea_newton_t s) { return s ? s->fmf.last : -1; }
// the last lambda_max estimates of the fine, vertex and third level (0 where there is none); out[3] = 1 if the last fine
// estimate ran its products through the matrix-free pair
extern "C" int tlfea_newton_get_lambda_max(tlfea_newton_t s, double out[4]) {
  if (!s || !out) return fail("null argument");
  out[0] = s->lam_max;
  out[1] = s->pmg.ok ? s->pmg.vertex.lam : 0.0;
  out[2] = s->pmg.agg.ok ? s->pmg.agg.lvl.lam : 0.0;
  out[3] = s->lmax_used_mf ? 1.0 : 0.0;
  return 0;
}
// Test hooks: the preconditioner as an operator (tests/test_gpu_precond_operator.py).  The set-up is the one of a solve
// (precond_setup stages 0 and 1 back to back, as the modal solve runs them) from cold lambda_max estimates; the warm state
// of the linear solver is put back afterwards, as tlfea_newton_modal_solve does.
extern "C" int tlfea_newton_apply_preconditioner_block(tlfea_newton_t s, int m, const double* R, double* Z) {
  if (!s || !R || !Z) return fail("tlfea_newton_apply_preconditioner: null argument");
  if (m < 1) return fail("tlfea_newton_apply_preconditioner: needs at least one vector");
  if (!s->d_H) return fail("tlfea_newton_apply_preconditioner: no assembled H");
  TRY(hessian_current(s));  // the hook's set-up and its operator are those of the CSR H
  if (dist_on(s)) return fail("tlfea_newton_apply_preconditioner: not available on a partitioned mesh (set_interface / set_halo is active)");
  if (s->lin.method == 1) return fail("tlfea_newton_apply_preconditioner: method = 1 (sparse direct) has no preconditioner");
  const size_t n = 3 * (size_t)s->N;
  ModalWork wk;
  LamKeep keep;
  double *dR = nullptr, *dZ = nullptr;
  TRY(wk.alloc(&dR, (size_t)m * n));
  TRY(wk.alloc(&dZ, (size_t)m * n));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(dR, R, (size_t)m * n * sizeof(double), hipMemcpyHostToDevice));
  TRY(keep.save(s, wk));  // cold estimates: the result depends on no earlier solve
  auto run = [&]() -> int {
    // start vector of the fine lambda_max estimate: the first vector, ones where that is zero (no estimate from nothing)
    bool zero = true;
    for (size_t k = 0; k < n && zero; k++) zero = R[k] == 0.0;
    if (zero) {
      std::vector<double> ones(n, 1.0);
      HIP_TRY(hipMemcpy(s->d_b, ones.data(), n * sizeof(double), hipMemcpyHostToDevice));
    } else {
      HIP_TRY(hipMemcpy(s->d_b, dR, n * sizeof(double), hipMemcpyDeviceToDevice));
    }
    TRY(precond_setup_whole(s, s->d_b, "tlfea_newton_apply_preconditioner"));
    for (int k = 0; k < m; k++) TRY(precond_apply(s, dR + k * n, dZ + k * n, part(s, 0), false));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(Z, dZ, (size_t)m * n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  };
  const int rc = run();
  const std::string why = rc ? api_error() : std::string();
  (void)hipStreamSynchronize(s->stream);
  s->hook_lam[0] = s->lam_max; s->hook_lam[1] = s->pmg.vertex.lam; s->hook_lam[2] = s->pmg.agg.lvl.lam;
  keep.restore();
  if (rc) api_error() = why;
  return rc;
}
extern "C" int tlfea_newton_apply_preconditioner(tlfea_newton_t s, const double* r, double* z) {
  return tlfea_newton_apply_preconditioner_block(s, 1, r, z);
}
extern "C" int tlfea_newton_preconditioner_state(tlfea_newton_t s, int* iout16, double* dout8, double* coef, int coef_cap) {
  if (!s || !iout16 || !dout8 || !coef) return fail("tlfea_newton_preconditioner_state: null argument");
  for (int k = 0; k < 16; k++) iout16[k] = 0;
  for (int k = 0; k < 8; k++) dout8[k] = 0.0;
  const int deg = cheb_degree_eff(s);
  const bool pmg = deg > 1 && precond_eff(s) == 2 && s->pmg.ok && s->pmg.d_coef;
  const bool l3 = pmg && s->pmg.agg.ok;
  iout16[0] = deg > 1 ? (pmg ? 2 : 1) : 0;
  iout16[1] = pmg ? (l3 ? 3 : 2) : 0;
  iout16[2] = deg;
  iout16[12] = pmg_smoother_kind();
  iout16[14] = blk12_now(s) ? 12 : 3;
  iout16[15] = cheb_bits_eff(s);
  int n_coef = 0;
  const double* src = nullptr;
  if (pmg) {
    const PmgTable t = pmg_table(s);
    iout16[3] = t.ks;
    iout16[4] = t.resid(); iout16[5] = t.restart(); iout16[6] = t.beta(); iout16[7] = t.coarse();
    iout16[8] = t.level3();
    iout16[9] = t.ks2;
    iout16[10] = t.kc;
    iout16[11] = t.k3;
    n_coef = t.size();
    src = s->pmg.d_coef;
  } else if (deg > 1) {
    n_coef = 2 * deg;
    src = s->d_coef;
  }
  if (n_coef > coef_cap) return fail("tlfea_newton_preconditioner_state: the coefficient table has " + std::to_string(n_coef) + " doubles, coef_cap is smaller");
  iout16[13] = n_coef;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (n_coef) HIP_TRY(hipMemcpy(coef, src, (size_t)n_coef * sizeof(double), hipMemcpyDeviceToHost));
  dout8[0] = s->lam_max; dout8[1] = s->pmg.vertex.lam; dout8[2] = s->pmg.agg.lvl.lam; dout8[3] = s->lam_safety;
  dout8[4] = s->hook_lam[0]; dout8[5] = s->hook_lam[1]; dout8[6] = s->hook_lam[2];
  return 0;
}
