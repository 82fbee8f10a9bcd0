// direct_api.hip -- the sparse direct solve of the Newton solver (lin.method == 1): the engine's multifrontal Cholesky
// (direct_kernels.hip, planned by mf_host.h) or rocSOLVER's re-factorisation, and the read-back hooks of the native plan.
#include <dlfcn.h>

#include "newton_handle.h"
#include "direct_host.h"

using namespace tlfea;

// ---- sparse direct solve: rocSOLVER's re-factorisation path in place of cuDSS (SyncedNewton.cu:995-1029 analysis once,
// :1103-1114 REFACTORIZATION + SOLVE per Newton iteration) ------------------------------------------------------------
// rocSOLVER (and the rocBLAS handle it needs) are resolved at run time, like RCCL: the default iterative path never
// depends on them.  rocsolver_dcsrrf_* re-factorise a matrix of FIXED pattern given the permutation and the pattern of
// its Cholesky factor, which direct_host.h computes once per mesh (nested dissection + symbolic factorisation).
namespace {
struct RocsolverApi {
  void* lib = nullptr;
  int (*blas_create)(void**) = nullptr;
  int (*blas_destroy)(void*) = nullptr;
  int (*blas_set_stream)(void*, hipStream_t) = nullptr;
  int (*rf_create)(void**, void*) = nullptr;
  int (*rf_destroy)(void*) = nullptr;
  int (*rf_set_mode)(void*, int) = nullptr;
  int (*analysis)(void*, int, int, int, int*, int*, double*, int, int*, int*, double*, int*, int*, double*, int, void*) = nullptr;
  int (*refactchol)(void*, int, int, int*, int*, double*, int, int*, int*, double*, int*, void*) = nullptr;
  int (*solve)(void*, int, int, int, int*, int*, double*, int*, int*, double*, int, void*) = nullptr;
};
RocsolverApi& rocsolver_api() {
  static RocsolverApi a;
  static bool tried = false;
  if (tried) return a;
  tried = true;
  for (const char* name : {"librocsolver.so.0", "librocsolver.so", "/opt/rocm/lib/librocsolver.so.0"}) {
    a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (a.lib) break;
  }
  if (!a.lib) return a;
  auto sym = [&](const char* n) { return dlsym(a.lib, n) ? dlsym(a.lib, n) : dlsym(RTLD_DEFAULT, n); };
  a.blas_create = (int (*)(void**))sym("rocblas_create_handle");
  a.blas_destroy = (int (*)(void*))sym("rocblas_destroy_handle");
  a.blas_set_stream = (int (*)(void*, hipStream_t))sym("rocblas_set_stream");
  a.rf_create = (int (*)(void**, void*))sym("rocsolver_create_rfinfo");
  a.rf_destroy = (int (*)(void*))sym("rocsolver_destroy_rfinfo");
  a.rf_set_mode = (int (*)(void*, int))sym("rocsolver_set_rfinfo_mode");
  a.analysis = (decltype(a.analysis))sym("rocsolver_dcsrrf_analysis");
  a.refactchol = (decltype(a.refactchol))sym("rocsolver_dcsrrf_refactchol");
  a.solve = (decltype(a.solve))sym("rocsolver_dcsrrf_solve");
  if (!a.blas_create || !a.blas_destroy || !a.blas_set_stream || !a.rf_create || !a.rf_destroy || !a.rf_set_mode ||
      !a.analysis || !a.refactchol || !a.solve)
    a.lib = nullptr;
  return a;
}
}  // namespace

void tlfea::direct_destroy(tlfea_newton_t s) {
  auto& m = s->direct;
  if (!m.tried) return;  // never used: do not resolve (dlopen) rocSOLVER / rocBLAS just to tear nothing down
  for (void* q : m.owned)
    if (q) (void)hipFree(q);
  if (m.backend == 0) {
    m = tlfea_newton_s::Direct();
    return;
  }
  RocsolverApi& a = rocsolver_api();
  if (m.rfinfo && a.lib) (void)a.rf_destroy(m.rfinfo);
  if (m.blas && a.lib) (void)a.blas_destroy(m.blas);
  void* pp[] = {m.d_ptrA, m.d_indA, m.d_ptrT, m.d_indT, m.d_pivQ, m.d_valT};
  for (void* q : pp)
    if (q) (void)hipFree(q);
  m = tlfea_newton_s::Direct();
}

// once per mesh: ordering + symbolic factor on the host, rocSOLVER's analysis on the device
#define DTRACE(msg)                                                          \
  do {                                                                       \
    if (std::getenv("TLFEA_DIRECT_TRACE")) {                                 \
      std::fprintf(stderr, "tlfea direct: %s\n", msg);                       \
      std::fflush(stderr);                                                   \
    }                                                                        \
  } while (0)
// the engine's own backend: plan on the host (mf_host.h), everything else on the device
template <typename T>
static int mf_upload(tlfea_newton_s::Direct& m, const std::vector<T>& h, const T** out) {
  T* p = nullptr;
  HIP_TRY(hipMalloc(&p, std::max<size_t>(1, h.size()) * sizeof(T)));
  m.owned.push_back(p);
  if (!h.empty()) HIP_TRY(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = p;
  return 0;
}
static int direct_prepare_native(tlfea_newton_t s, const std::vector<double>& X) {
  auto& m = s->direct;
  tlfea_t10_t d = s->d;
  const int N = s->N;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  static const long long forced = env_ll("TLFEA_DIRECT_MAX_NNZ", 0);
  const long long max_doubles = forced > 0 ? forced : (long long)(0.8 * (double)free_b / sizeof(double));
  static const int leaf = env_int("TLFEA_DIRECT_LEAF", 32);
  if (!mf_plan_build(N, d->h_off.data(), d->h_cols.data(), X.data(), X.data() + N, X.data() + 2 * (size_t)N, leaf, max_doubles,
                     m.plan))
    return fail("sparse direct solve: the Cholesky factor and front workspaces of this mesh do not fit the device memory "
                "that is free (TLFEA_DIRECT_MAX_NNZ overrides the bound, in doubles); use the iterative solver");
  const MfPlan& P = m.plan;
  std::vector<MfFrontDev> fr(P.fronts.size());
  for (size_t f = 0; f < P.fronts.size(); f++) {
    const MfFront& F = P.fronts[f];
    fr[f] = MfFrontDev{F.F_off, F.L_off, F.v_off, F.map_off, F.row_off, F.cF_off, 3 * F.nrows, 3 * (F.c1 - F.c0), F.c0,
                       F.child[0], F.child[1], F.c_ld, F.c_k0, 0};
  }
  MfDev& D = m.dev;
  TRY(mf_upload(m, fr, &D.fr));
  TRY(mf_upload(m, P.level_fronts, &D.lvl));
  TRY(mf_upload(m, P.batch_fronts, &D.blvl));
  TRY(mf_upload(m, P.map, &D.map));
  TRY(mf_upload(m, P.rows, &D.rows));
  TRY(mf_upload(m, P.order, &D.order));
  TRY(mf_upload(m, P.h_src, &D.hsrc));
  TRY(mf_upload(m, P.h_dst, &D.hdst));
  TRY(mf_upload(m, P.h_sld, &D.hsld));
  TRY(mf_upload(m, P.h_dld, &D.hdld));
  auto dalloc = [&](double** p, long long n) {
    HIP_TRY(hipMalloc(p, (size_t)std::max(1LL, n) * sizeof(double)));
    m.owned.push_back(*p);
    return 0;
  };
  TRY(dalloc(&D.L, P.L_total));
  for (int t = 0; t < 4; t++) TRY(dalloc(&D.F[t], P.F_cap[t]));
  TRY(dalloc(&D.v, P.v_total));
  TRY(dalloc(&D.y, 3LL * N));
  TRY(dalloc(&D.xp, 3LL * N));
  HIP_TRY(hipMalloc(&D.err, sizeof(int)));
  m.owned.push_back(D.err);
  m.n = 3 * N;
  m.ok = true;
  if (s->verbose || std::getenv("TLFEA_DIRECT_TRACE"))
    std::printf("sparse direct solve: %d DOF, %zu fronts in %d levels, factor %.3g doubles (%.1f x the lower triangle of H), "
                "workspaces %.3g doubles (fronts down to depth %d one by one with a stack), %.3g flop per factorisation\n",
                m.n, P.fronts.size(), P.n_levels(), (double)P.L_total, (double)P.L_total / (0.5 * s->h_nnz),
                (double)P.F_total(), P.top_depth, (double)P.flops);
  return 0;
}

static int direct_prepare(tlfea_newton_t s) {
  auto& m = s->direct;
  if (m.tried) return m.ok ? 0 : fail("sparse direct solve is not available (see the earlier message)");
  m.tried = true;
  tlfea_t10_t d = s->d;
  if (dist_on(s)) return fail("sparse direct solve: single-GPU path only");
  {
    const char* be = std::getenv("TLFEA_DIRECT_BACKEND");
    m.backend = (be && std::string(be) == "rocsolver") ? 1 : 0;
  }
  // coordinates of the coefficient vectors for the dissection planes (ANCF: the 4 vectors of a node share its position)
  const int N = s->N;
  std::vector<double> X(3 * (size_t)N);
  D2H(X.data(), d->d_xt, (size_t)N);
  D2H(X.data() + N, d->d_yt, (size_t)N);
  D2H(X.data() + 2 * (size_t)N, d->d_zt, (size_t)N);
  if (d->kind != kT10)
    for (int i = 0; i < N; i++)
      for (int c = 0; c < 3; c++) X[(size_t)c * N + i] = X[(size_t)c * N + (i / 4) * 4];
  if (m.backend == 0) return direct_prepare_native(s, X);
  DTRACE("resolving rocsolver");
  RocsolverApi& a = rocsolver_api();
  DTRACE("resolved");
  if (!a.lib) return fail("sparse direct solve: librocsolver / librocblas could not be resolved at run time");
  DirectHost h;
  static const long long max_nnz = env_ll("TLFEA_DIRECT_MAX_NNZ", 400000000LL);
  if (!direct_symbolic(N, d->h_off.data(), d->h_cols.data(), X.data(), X.data() + N, X.data() + 2 * (size_t)N, max_nnz, h))
    return fail("sparse direct solve: the Cholesky factor of this mesh exceeds the size limit (TLFEA_DIRECT_MAX_NNZ, default "
                "4e8 entries = 3.2 GB); use the iterative solver");
  m.n = h.n;
  m.nnzT = (int)h.indT.size();
  TRY(dmalloc(&m.d_ptrA, s->h_row_offsets.size()));
  TRY(dmalloc(&m.d_indA, s->h_col_indices.size()));
  TRY(dmalloc(&m.d_ptrT, h.ptrT.size()));
  TRY(dmalloc(&m.d_indT, h.indT.size()));
  TRY(dmalloc(&m.d_pivQ, h.perm.size()));
  TRY(dmalloc(&m.d_valT, h.indT.size()));
  HIP_TRY(hipMemcpy(m.d_ptrA, s->h_row_offsets.data(), s->h_row_offsets.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m.d_indA, s->h_col_indices.data(), s->h_col_indices.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m.d_ptrT, h.ptrT.data(), h.ptrT.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m.d_indT, h.indT.data(), h.indT.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m.d_pivQ, h.perm.data(), h.perm.size() * sizeof(int), hipMemcpyHostToDevice));
  {  // a valid factor for the analysis phase (it inspects the pattern): the identity on T's pattern
    std::vector<double> vT(h.indT.size(), 0.0);
    for (int r = 0; r < h.n; r++) vT[(size_t)h.ptrT[r + 1] - 1] = 1.0;  // the diagonal is the last entry of a row
    HIP_TRY(hipMemcpy(m.d_valT, vT.data(), vT.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  DTRACE("symbolic done, creating rocblas handle");
  if (a.blas_create(&m.blas)) return fail("rocblas_create_handle failed");
  DTRACE("handle created");
  if (a.blas_set_stream(m.blas, s->stream)) return fail("rocblas_set_stream failed");
  if (a.rf_create(&m.rfinfo, m.blas)) return fail("rocsolver_create_rfinfo failed");
  if (a.rf_set_mode(m.rfinfo, /*rocsolver_rfinfo_mode_cholesky*/ 272)) return fail("rocsolver_set_rfinfo_mode failed");
  DTRACE("rfinfo ready, analysis");
  const int rc = a.analysis(m.blas, m.n, 1, s->h_nnz, m.d_ptrA, m.d_indA, s->d_H, m.nnzT, m.d_ptrT, m.d_indT, m.d_valT,
                            nullptr, m.d_pivQ, s->d_dv, m.n, m.rfinfo);
  if (rc) return fail("rocsolver_dcsrrf_analysis failed with status " + std::to_string(rc));
  HIP_TRY(hipStreamSynchronize(s->stream));
  DTRACE("analysis done");
  m.ok = true;
  if (s->verbose)
    std::printf("sparse direct solve: %d DOF, factor %d entries (%.1f x the lower triangle of H), nested dissection\n", m.n,
                m.nnzT, (double)m.nnzT / (0.5 * s->h_nnz));
  return 0;
}

// H x = b by re-factorisation + triangular solves; the true residual is measured with the fp64 SpMV of the CG
int tlfea::direct_solve(tlfea_newton_t s, const double* d_b, double* d_x, int* iters_out, double* rel_out) {
  TRY(hessian_current(s));  // the factorisation and the residual's SpMV read H
  TRY(direct_prepare(s));
  auto& m = s->direct;
  static RocsolverApi none;
  RocsolverApi& a = m.backend == 1 ? rocsolver_api() : none;
  tlfea_t10_t d = s->d;
  StageTimer t(s, 4);
  const size_t nb = (size_t)m.n * sizeof(double);
  if (m.backend == 0) {
    launch_mf_factor(s->stream, m.plan, m.dev, s->d_H, m.tally);
    launch_mf_solve(s->stream, m.plan, m.dev, d_b, d_x, m.tally);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, m.dev.err, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    if (bad) return fail("sparse direct solve: a pivot of the Cholesky factorisation is not positive (H not positive definite)");
  } else {
  int rc = a.refactchol(m.blas, m.n, s->h_nnz, m.d_ptrA, m.d_indA, s->d_H, m.nnzT, m.d_ptrT, m.d_indT, m.d_valT, m.d_pivQ,
                        m.rfinfo);
  if (rc) return fail("rocsolver_dcsrrf_refactchol failed with status " + std::to_string(rc) + " (H not positive definite?)");
  DTRACE("refactchol enqueued");
  HIP_TRY(hipMemcpyAsync(d_x, d_b, nb, hipMemcpyDeviceToDevice, s->stream));
  rc = a.solve(m.blas, m.n, 1, m.nnzT, m.d_ptrT, m.d_indT, m.d_valT, nullptr, m.d_pivQ, d_x, m.n, m.rfinfo);
  if (rc) return fail("rocsolver_dcsrrf_solve failed with status " + std::to_string(rc));
  DTRACE("solve enqueued");
  }
  // r = b - H x, ||r|| / ||b||
  HIP_TRY(hipMemsetAsync(s->d_parts, 0, (size_t)5 * kNPart * sizeof(double), s->stream));
  launch_spmv_dir_dot(s->stream, s->N, d->inc(), s->d_H, d_x, s->d_p, 1, part(s, 1), part(s, 0), s->d_p2, s->d_q, part(s, 2),
                      true, s->spmv_nt);
  launch_diff(s->stream, m.n, d_b, s->d_q, s->d_r);
  double rr = 0.0, bb = 0.0;
  launch_norm2(s->stream, s->d_r, nullptr, m.n, part(s, 5), s->d_scal);
  launch_norm2(s->stream, d_b, nullptr, m.n, part(s, 4), s->d_scal + 1);
  TRY(fetch_scalar2(s, s->d_scal, &rr, &bb));
  HIP_TRY(hipGetLastError());
  t.stop();
  const double rel = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
  if (iters_out) *iters_out = 1;
  if (rel_out) *rel_out = rel;
  // a backward-stable factorisation leaves ||r||/||b|| at a few ulp times the growth of the factor: the tolerance of the
  // iterative path does not apply; what is reported (and tested) is the measured residual
  s->lin_last_rel = rel;
  s->lin_last_ok = rel == rel && rel <= 1e-8;
  s->lin_worst_rel = (rel != rel) ? rel : std::max(s->lin_worst_rel, rel);
  s->lin_all_ok = s->lin_all_ok && s->lin_last_ok;
  if (!s->lin_last_ok && !s->lin.on_unconverged) {
    char msg[200];
    std::snprintf(msg, sizeof msg, "sparse direct solve left ||r||/||b|| = %.3e (H not positive definite, or ill-conditioned "
                  "beyond fp64)", rel);
    return fail(msg);
  }
  return 0;
}

// Test hooks of the native sparse direct solve: the plan the solver holds and the launches its last factorisation + solve
// issued (host counters next to the launches, direct_kernels.hip), so that a test can assert which kernels a mesh and the
// TLFEA_DIRECT_* switches reached.  Available once a direct solve has built the plan.
extern "C" int tlfea_newton_get_direct_info(tlfea_newton_t s, long long* out22) {
  if (!s || !out22) return fail("tlfea_newton_get_direct_info: null argument");
  const auto& m = s->direct;
  if (!m.ok || m.backend != 0) return fail("tlfea_newton_get_direct_info: no native direct solve has run on this solver");
  const MfPlan& P = m.plan;
  long long m_max = 0, k_max = 0, k_zero = 0;
  for (const MfFront& F : P.fronts) {
    m_max = std::max(m_max, 3LL * F.nrows);
    k_max = std::max(k_max, 3LL * (F.c1 - F.c0));
    k_zero += F.c1 == F.c0;
  }
  const MfTally& t = m.tally;
  const long long v[22] = {(long long)P.fronts.size(), P.n_levels(), P.top_depth, P.L_total, P.F_cap[0], P.F_cap[1], P.F_cap[2],
                           P.F_cap[3], m_max, k_max, k_zero, P.N, t.panel, t.update_inner, t.update_trailing, t.update_wide,
                           t.extend_add, t.push, t.levels_one_wg, t.levels_stepwise, t.fwd_step, t.bwd_step};
  std::copy(v, v + 22, out22);
  return 0;
}
extern "C" int tlfea_newton_get_direct_fronts(tlfea_newton_t s, int* order, int* fronts7) {
  if (!s || !order || !fronts7) return fail("tlfea_newton_get_direct_fronts: null argument");
  const auto& m = s->direct;
  if (!m.ok || m.backend != 0) return fail("tlfea_newton_get_direct_fronts: no native direct solve has run on this solver");
  const MfPlan& P = m.plan;
  std::copy(P.order.begin(), P.order.end(), order);
  for (size_t f = 0; f < P.fronts.size(); f++) {
    const MfFront& F = P.fronts[f];
    const int v[7] = {F.c0, F.c1, F.depth, F.parent, F.nrows, F.child[0], F.child[1]};
    std::copy(v, v + 7, fronts7 + 7 * f);
  }
  return 0;
}
