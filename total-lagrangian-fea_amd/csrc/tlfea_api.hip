// tlfea_api.hip -- C-ABI (include/tlfea_c.h) over the gfx950 kernels: buffer ownership, the host
// side of the sparsity analysis, and the ALM/Newton control flow of the reference
// (SyncedNewton.cu:909-1146) around the device PCG (cg_api.hip, precond_api.hip) that stands in place of cuDSS.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "newton_handle.h"
#include "pmg_coef.h"
#include "rowgroup_host.h"
#include "vbd_host.h"

using namespace tlfea;

std::string& tlfea::api_error() {
  thread_local std::string err;
  return err;
}
extern "C" const char* tlfea_last_error(void) { return api_error().c_str(); }
// every C-ABI translation unit reports through this one message
int tlfea::api_fail(const std::string& msg) {
  api_error() = msg;
  std::fprintf(stderr, "tlfea: %s\n", msg.c_str());
  return 1;
}
extern "C" int tlfea_version(void) { return 100; }
extern "C" int tlfea_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int tlfea_newton_create(tlfea_t10_t data, int n_constraints, tlfea_newton_t* out) {
  if (!data || !out) return fail("tlfea_newton_create: null argument");
  // The reference sizes lambda from this count and indexes it with the data object's constraint ids: any other value
  // than the data object's own count (or 0 = constraint terms off, SyncedNewton.cu "if (n_constraints_ > 0)") would
  // read and write past the multipliers.
  if (n_constraints != 0 && n_constraints != data->n_constraint)
    return fail("solver n_constraints (" + std::to_string(n_constraints) + ") differs from the data object's (" +
                std::to_string(data->n_constraint) + "): pass data.get_n_constraint()");
  auto* s = new tlfea_newton_s();
  s->d = data;
  s->N = data->N;
  s->cons_enabled = n_constraints > 0;
  s->n_constraints = n_constraints;
  s->n_constraints_global = n_constraints;
  const size_t n = 3 * (size_t)s->N;
  TRY(dmalloc(&s->d_v, n)); TRY(dmalloc(&s->d_vprev, n)); TRY(dmalloc(&s->d_g, n)); TRY(dmalloc(&s->d_dv, n));
  TRY(dmalloc(&s->d_r, n)); TRY(dmalloc(&s->d_b, n)); TRY(dmalloc(&s->d_eigv, n)); TRY(dmalloc(&s->d_cd, n));
  TRY(dmalloc(&s->d_cd2, n)); TRY(dmalloc(&s->d_cres, n)); TRY(dmalloc(&s->d_p, n)); TRY(dmalloc(&s->d_p2, n)); TRY(dmalloc(&s->d_q, n)); TRY(dmalloc(&s->d_zv, n));
  TRY(dmalloc(&s->d_lam, (size_t)std::max(1, n_constraints)));
  TRY(dmalloc(&s->d_xp, (size_t)s->N)); TRY(dmalloc(&s->d_yp, (size_t)s->N)); TRY(dmalloc(&s->d_zp, (size_t)s->N));
  TRY(dmalloc(&s->d_parts, (size_t)6 * kNPart));
  TRY(dmalloc(&s->d_scal, (size_t)4));
  HIP_TRY(hipHostMalloc((void**)&s->h_pin, (8 + kPmgTableCap) * sizeof(double)));
  TRY(dmalloc(&s->d_coef, (size_t)2 * kChebMaxDeg));
  s->use_graphs = env_flag("TLFEA_GRAPH", s->use_graphs);
  TRY(dmalloc(&s->d_Dinv, (size_t)9 * s->N));
  TRY(dmalloc(&s->d_D, (size_t)9 * s->N));
  TRY(dmalloc(&s->d_f32, (size_t)6 * n + (size_t)9 * s->N));
  TRY(dmalloc(&s->d_sc, n)); TRY(dmalloc(&s->d_cz, n)); TRY(dmalloc(&s->d_cz2, n)); TRY(dmalloc(&s->d_cres2, n));
  TRY(dmalloc(&s->d_Dinv_s, (size_t)9 * s->N));
  for (auto& e : s->ev) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(hipStreamCreate(&s->stream_own));
  s->stream = s->stream_own;
  s->pcg_fused = env_int("TLFEA_PCG_FUSED", s->pcg_fused);
  if (const char* e = std::getenv("TLFEA_SPMV32")) s->spmv32_every = std::max(0, std::atoi(e)) & ~1;  // even: odd parity
  if (const char* e = std::getenv("TLFEA_CHEB_DEG")) s->lin.cheb_degree = std::min(kChebMaxDeg, std::max(0, std::atoi(e)));
  s->spmv_nt = env_flag("TLFEA_SPMV_NT", s->spmv_nt);
  s->lin.cheb_bits = env_int("TLFEA_CHEB_BITS", s->lin.cheb_bits);
  s->lin.precond = env_int("TLFEA_PRECOND", s->lin.precond);
  if (const char* e = std::getenv("TLFEA_ASSEMBLE"))
    s->asm_mode = (std::string(e) == "kbuf") ? 1 : (std::string(e) == "general") ? 2 : 0;
  if (const char* e = std::getenv("TLFEA_MASS")) s->mass_mode = (std::string(e) == "csr") ? 1 : 0;
  *out = s;
  return tlfea_newton_setup(s);
}

extern "C" int tlfea_newton_destroy(tlfea_newton_t s) {
  if (!s) return 0;
  void* ptrs[] = {s->d_v, s->d_vprev, s->d_lam, s->d_g, s->d_dv, s->d_r, s->d_b, s->d_eigv, s->d_cd, s->d_cd2, s->d_cres, s->d_xp, s->d_yp, s->d_zp, s->d_H,
                  s->d_Kbuf, s->d_Dinv, s->d_p, s->d_p2, s->d_q, s->d_zv, s->d_parts, s->d_scal, s->d_if_node, s->d_if_slot, s->d_ibuf, s->d_w, s->d_nw, s->d_wc, s->d_D, s->d_B8, s->d_B1, s->d_sc, s->d_Dinv_s, s->d_cz, s->d_cz2, s->d_cres2, s->d_f32, s->d_own, s->d_sc_mask, s->d_step0, s->d_lam0, s->d_H32};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (int* p : s->d_rg)
    if (p) (void)hipFree(p);
  for (int* p : s->d_rg4)
    if (p) (void)hipFree(p);
  if (s->d_L12inv) (void)hipFree(s->d_L12inv);
  if (s->d_L12inv_f) (void)hipFree(s->d_L12inv_f);
  if (s->d_blk12_err) (void)hipFree(s->d_blk12_err);
  if (s->d_gvec) (void)hipFree(s->d_gvec);
  if (s->d_cmass) (void)hipFree(s->d_cmass);
  if (s->d_Fq) (void)hipFree(s->d_Fq);
  if (s->d_mbuf) (void)hipFree(s->d_mbuf);
  if (s->mf.d_ybuf) (void)hipFree(s->mf.d_ybuf);
  if (s->mf.d_gp) (void)hipFree(s->mf.d_gp);
  if (s->mf.d_Fp) (void)hipFree(s->mf.d_Fp);
  if (s->fmf.d_g32) (void)hipFree(s->fmf.d_g32);
  if (s->fmf.d_F32) (void)hipFree(s->fmf.d_F32);
  if (s->fmf.d_scn) (void)hipFree(s->fmf.d_scn);
  if (s->fmf.d_ss) (void)hipFree(s->fmf.d_ss);
  for (void* p : s->mf.d_cp)
    if (p) (void)hipFree(p);
  {
    auto& r = s->sr;
    void* rp[] = {r.d_rg[0], r.d_rg[1], r.d_rg[2], r.d_rg[3], r.d_rg[4], r.d_cmass4, r.d_ch_row, r.d_ch_pos, r.d_id_off, r.d_id_ch,
                  r.d_id_w, r.d_id_pos, r.d_img, r.d_dbuf};
    for (void* p : rp)
      if (p) (void)hipFree(p);
  }
  direct_destroy(s);
  for (auto& e : s->ev)
    if (e) (void)hipEventDestroy(e);
  if (s->h_pin) (void)hipHostFree(s->h_pin);
  cg_graphs_destroy(s);
  {
    auto& m = s->pmg;
    void* pd[] = {m.d_ifc_node, m.d_ifc_slot, m.d_bslot_c, m.d_wc3, m.d_child_w_dist, s->d_bslot_f};
    for (void* q : pd)
      if (q) (void)hipFree(q);
    void* pp[] = {m.d_par0, m.d_par1, m.d_cblk_row, m.d_child_off, m.d_child, m.d_con_off, m.d_con_base, m.d_con_deg,
                  m.d_child_w, m.d_con_w, m.d_coef, m.d_c_upper, m.d_c_mirror};
    for (void* q : pp)
      if (q) (void)hipFree(q);
    m.vertex.release();
    auto& ro = m.rop;
    void* rr[] = {ro.d_off, ro.d_cols, ro.d_ch_off, ro.d_ch, ro.d_con_off, ro.d_con_blk, ro.d_con_ord, ro.d_ch_w, ro.d_R1,
                  ro.d_R8, ro.d_pos_off, ro.d_con_pos};
    for (void* q : rr)
      if (q) (void)hipFree(q);
    auto& gr = m.rows;
    void* gq[] = {gr.d_row, gr.d_off, gr.d_long_rows, gr.d_pos, gr.d_w, gr.d_ws};
    for (void* q : gq)
      if (q) (void)hipFree(q);
    auto& g = m.agg;
    void* gg[] = {g.d_agg, g.d_active, g.d_mem_off, g.d_mem, g.d_pair_A, g.d_pair_pos, g.d_pair_B, g.d_pcon_off,
                  g.d_pcon_base, g.d_pcon_deg, g.d_pcon_i, g.d_pcon_j, g.d_rvec, g.d_r3};
    for (void* q : gg)
      if (q) (void)hipFree(q);
    g.lvl.release();
  }
  if (s->d_coef) (void)hipFree(s->d_coef);
  {
    auto& h = s->halo;
    halo_free_plans(h.lv[0]);
    halo_free_plans(h.lv[1]);
    if (h.d_sbuf) (void)hipFree(h.d_sbuf);
    if (h.d_rbuf) (void)hipFree(h.d_rbuf);
    if (h.d_red) (void)hipFree(h.d_red);
    if (h.ev0) (void)hipEventDestroy(h.ev0);
    if (h.ev1) (void)hipEventDestroy(h.ev1);
  }
  if (s->stream_own) (void)hipStreamDestroy(s->stream_own);
  delete s;
  return 0;
}

extern "C" int tlfea_newton_setup(tlfea_newton_t s) {  // SyncedNewton.cuh:231-245
  const size_t n = 3 * (size_t)s->N;
  HIP_TRY(hipMemset(s->d_v, 0, n * sizeof(double)));
  HIP_TRY(hipMemset(s->d_vprev, 0, n * sizeof(double)));
  HIP_TRY(hipMemset(s->d_g, 0, n * sizeof(double)));
  HIP_TRY(hipMemset(s->d_dv, 0, n * sizeof(double)));
  HIP_TRY(hipMemset(s->d_lam, 0, (size_t)std::max(1, s->n_constraints) * sizeof(double)));
  HIP_TRY(hipMemset(s->d_xp, 0, (size_t)s->N * sizeof(double)));
  HIP_TRY(hipMemset(s->d_yp, 0, (size_t)s->N * sizeof(double)));
  HIP_TRY(hipMemset(s->d_zp, 0, (size_t)s->N * sizeof(double)));
  return 0;
}
extern "C" int tlfea_newton_set_parameters(tlfea_newton_t s, const tlfea_newton_params* p) {
  if (!s || !p) return fail("null argument");
  s->prm = *p;
  return 0;
}
extern "C" int tlfea_newton_set_linsolve_opts(tlfea_newton_t s, const tlfea_linsolve_opts* o) {
  if (!s || !o) return fail("null argument");
  s->lin = *o;
  if (s->lin.check_every < 1) s->lin.check_every = 1;
  if (s->lin.cheb_degree < 0) s->lin.cheb_degree = 0;
  if (s->lin.cheb_degree > kChebMaxDeg) s->lin.cheb_degree = kChebMaxDeg;
  if (!(s->lin.cheb_kappa > 1.0)) s->lin.cheb_kappa = 0.0;  // auto
  if (s->lin.cheb_bits != 16 && s->lin.cheb_bits != 32 && s->lin.cheb_bits != 64) s->lin.cheb_bits = 0;
  if (s->lin.precond < 0 || s->lin.precond > 2) s->lin.precond = 0;
  s->lin.on_unconverged = s->lin.on_unconverged ? 1 : 0;
  s->lin.method = s->lin.method == 1 ? 1 : 0;
  return 0;
}
extern "C" int tlfea_newton_set_fixed_sparsity_pattern(tlfea_newton_t s, int fixed) {
  s->fixed_pattern = fixed != 0;
  return 0;
}
extern "C" int tlfea_newton_set_verbose(tlfea_newton_t s, int v) {
  s->verbose = v;
  return 0;
}
extern "C" int tlfea_newton_set_profiling(tlfea_newton_t s, int on) {
  s->profiling = on != 0;
  return 0;
}
extern "C" double* tlfea_newton_velocity_guess_device_ptr(tlfea_newton_t s) { return s->d_v; }

// DOF-level CSR pattern from the coefficient adjacency (SyncedNewton.cu:163-205,830-897)

// ---- work lists of the fused tangent + assembly kernel (T10) -------------------------------------------------------------
// Both functions can run again after CalcDnDuPre re-referenced the mesh (refresh_geometry): the affine form's vertex
// gradients, det J and its 'every element is straight-sided' decision are derived from the grad N / det J of ONE call.
// per-point F records of the residual launch: [E][5][10] (affine form) or [E][Q][9] (general form) -- one buffer fits both
// (the material, hence the form, may be switched between solves)
static int ensure_fq(tlfea_newton_t s) {
  if (s->d_Fq) return 0;
  tlfea_t10_t d = s->d;
  return dmalloc(&s->d_Fq, std::max((size_t)d->Epad * 50, (size_t)d->E * d->Q * 9));
}
// Affine form: every element straight-sided (checked on the device against the stored grad N / det J) and the rule the
// 5-point Keast rule (L = 1/4 at one point, one vertex at 1/2 and three at 1/6 at the others).
static int setup_affine_form(tlfea_newton_t s, bool* affine_out) {
  tlfea_t10_t d = s->d;
  const int N = s->N;
  *affine_out = false;
  s->affine_ok = false;
  s->mf.valid = false;
  if (!(s->asm_mode == 0 && d->have_dndu)) return 0;
  AffineView av{nullptr, -1, {-1, -1, -1, -1}};
  bool rule_ok = true;
  for (int q = 0; q < kNQ && rule_ok; q++) {
    const double L[4] = {1.0 - d->h_q[0][q] - d->h_q[1][q] - d->h_q[2][q], d->h_q[0][q], d->h_q[1][q], d->h_q[2][q]};
    int n4 = 0, n2 = 0, n6 = 0, v2 = -1;
    for (int k = 0; k < 4; k++) {
      if (std::fabs(L[k] - 0.25) < 1e-14) n4++;
      else if (std::fabs(L[k] - 0.5) < 1e-14) n2++, v2 = k;
      else if (std::fabs(L[k] - 1.0 / 6.0) < 1e-14) n6++;
    }
    if (n4 == 4 && av.q0 < 0) av.q0 = q;
    else if (n2 == 1 && n6 == 3 && av.qv[v2] < 0) av.qv[v2] = q;
    else rule_ok = false;
  }
  // the kernel evaluates the four outer points in a lane-relative order: they must carry one weight (Keast: 9/20 x 1/6)
  for (int p = 1; p < 4 && rule_ok; p++)
    if (std::fabs(d->h_qw[av.qv[p]] - d->h_qw[av.qv[0]]) > 1e-15 * std::fabs(d->h_qw[av.qv[0]])) rule_ok = false;
  if (!rule_ok) return 0;
  double* d_dev = nullptr;
  if (!s->d_gvec) TRY(dmalloc(&s->d_gvec, (size_t)d->E * 16));
  TRY(dmalloc(&d_dev, 1));
  HIP_TRY(hipMemsetAsync(d_dev, 0, sizeof(double), d->stream));
  av.gvec = s->d_gvec;
  s->fmf.g_ok = false;
  s->mf.gp_ok = false;
  launch_affine_pre(d->stream, d->view(), av, s->d_gvec, d_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(d->stream));
  D2H(&s->affine_dev, d_dev, 1);
  if (std::getenv("TLFEA_AF_VERBOSE"))
    std::fprintf(stderr, "affine check: largest relative deviation of grad N / det J from the affine form %.3e\n", s->affine_dev);
  (void)hipFree(d_dev);
  if (!(s->affine_dev <= 1e-12)) return 0;
  if (!s->d_rg4[0]) {  // the work lists depend on the connectivity only: built once
    RowGroups4Host rh;
    if (!build_row_groups4(N, d->E, d->h_conn.data(), d->h_off.data(), d->h_cols.data(), d->h_n2e_off.data(),
                           d->h_n2e.data(), d->h_X0.data(), d->h_X0.data() + N, d->h_X0.data() + 2 * (size_t)N, rh))
      return 0;
    // a group's accumulator plus the kernel's staging must fit a workgroup's LDS (the builder only knows its 16-bit packing)
    if (assemble_affine_lds_max(rh.acc_max) > device_lds_limit()) return 0;
    s->rg4_passes = (int)(rh.pt.size() / 4);
    const std::vector<int>* src[5] = {&rh.g_pass_off, &rh.pt, &rh.gr_info, &rh.gi_head, &rh.gi_ent};
    for (int k = 0; k < 5; k++) {
      TRY(dmalloc(&s->d_rg4[k], src[k]->size() + 4));
      HIP_TRY(hipMemcpy(s->d_rg4[k], src[k]->data(), src[k]->size() * sizeof(int), hipMemcpyHostToDevice));
    }
    s->rg4 = RowGroups4{rh.G(), d->E * d->S, rh.acc_max, s->d_rg4[0], reinterpret_cast<const int4*>(s->d_rg4[1]),
                        reinterpret_cast<const int4*>(s->d_rg4[2]), reinterpret_cast<const int2*>(s->d_rg4[3]),
                        reinterpret_cast<const int2*>(s->d_rg4[4])};
  }
  s->av = av;
  if (!s->d_cmass) {  // element mass coefficients C_ij = sum_q w_q N_i(q) N_j(q) (the rule of FEAT10Data.cu:206-278)
    const int edges[6][2] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {1, 3}, {2, 3}};  // FEAT10Data.cu:143
    double Nq[kNQ][kNN], cm[160];
    for (int q = 0; q < kNQ; q++) {
      const double L[4] = {1.0 - d->h_q[0][q] - d->h_q[1][q] - d->h_q[2][q], d->h_q[0][q], d->h_q[1][q], d->h_q[2][q]};
      for (int k = 0; k < 4; k++) Nq[q][k] = L[k] * (2.0 * L[k] - 1.0);
      for (int k = 0; k < 6; k++) Nq[q][k + 4] = 4.0 * L[edges[k][0]] * L[edges[k][1]];
    }
    for (int il = 0; il < kNN; il++)
      for (int n = 0; n < 4; n++)
        for (int p = 0; p < 4; p++) {
          const int j = p == n ? n : t10_mid_of(n, p);
          double c = 0.0;
          for (int q = 0; q < kNQ; q++) c += d->h_qw[q] * Nq[q][il] * Nq[q][j];
          cm[il * 16 + 4 * n + p] = p == n ? c : 0.5 * c;
        }
    TRY(dmalloc(&s->d_cmass, 160));
    HIP_TRY(hipMemcpy(s->d_cmass, cm, sizeof(cm), hipMemcpyHostToDevice));
  }
  TRY(ensure_fq(s));  // [E][5][10]: F per point, centroid point first
  s->rg_ok = s->affine_ok = *affine_out = true;
  return 0;
}
// General form (curved elements, other rules): reads the stored grad N itself, nothing to refresh.
static int setup_general_form(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  const int N = s->N;
  s->rg_ok = false;
  if (!s->d_rg[0]) {
    RowGroupsHost rh;
    if (!build_row_groups(N, d->E, d->S, d->h_conn.data(), d->h_off.data(), d->h_cols.data(), d->h_n2e_off.data(),
                          d->h_n2e.data(), d->h_X0.data(), d->h_X0.data() + N, d->h_X0.data() + 2 * (size_t)N, rh))
      return 0;
    if (assemble_direct_lds_max(rh.acc_max) > device_lds_limit()) return 0;  // as setup_affine_form: the two-kernel path is next
    s->rg_passes = (int)(rh.pt.size() / 4);
    const std::vector<int>* src[6] = {&rh.g_pass_off, &rh.pt, &rh.gr_info, &rh.gi_code, &rh.gi_mb, &rh.gi_pack};
    for (int k = 0; k < 6; k++) {
      TRY(dmalloc(&s->d_rg[k], src[k]->size() + 4));
      HIP_TRY(hipMemcpy(s->d_rg[k], src[k]->data(), src[k]->size() * sizeof(int), hipMemcpyHostToDevice));
    }
    s->rg = RowGroups{rh.G(), d->E * d->S, rh.acc_max, s->d_rg[0], reinterpret_cast<const int4*>(s->d_rg[1]),
                      reinterpret_cast<const int4*>(s->d_rg[2]), s->d_rg[3], s->d_rg[4], s->d_rg[5]};
  }
  TRY(ensure_fq(s));
  s->rg_ok = true;
  return 0;
}
// CalcDnDuPre ran again since the work lists were built (re-referencing after UpdatePositions, which the reference
// API permits): redo the affine extraction and the straight-sidedness check from the new grad N / det J, and fall
// back to the general form if the new reference configuration is curved.
static int refresh_geometry(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  if (!s->sparsity_done || s->geom_gen_seen < 0 || d->geom_gen == s->geom_gen_seen) return 0;
  HIP_TRY(hipStreamSynchronize(s->stream));
  bool affine = false;
  TRY(setup_affine_form(s, &affine));
  if (!affine) TRY(setup_general_form(s));
  s->geom_gen_seen = d->geom_gen;
  return 0;
}

extern "C" int tlfea_newton_analyze_hessian_sparsity(tlfea_newton_t s) {
  if (s->sparsity_done) return 0;
  tlfea_t10_t d = s->d;
  TRY(tlfea_t10_build_mass_csr_pattern(d));
  const int N = s->N;
  // The longest node row must fit a workgroup's LDS in assemble_rows_kernel, the form every mesh can fall back to (the fused
  // forms need more than that for the same row).  Checked before anything of the solver changes and before any launch.
  if (assemble_rows_lds(d->maxdeg) > device_lds_limit()) {
    int worst = 0;
    for (int i = 0; i < N; i++)
      if (d->h_off[i + 1] - d->h_off[i] == d->maxdeg) {
        worst = i;
        break;
      }
    return fail("tlfea_newton_analyze_hessian_sparsity: node " + std::to_string(worst) + " has " + std::to_string(d->maxdeg) +
                " neighbours: its row of H needs " + std::to_string(assemble_rows_lds(d->maxdeg)) +
                " bytes of LDS in the assembly, a workgroup of this device has " + std::to_string(device_lds_limit()));
  }
  s->iso_first = -1;
  s->iso_count = 0;
  for (int i = 0; i < N; i++)
    if (d->h_off[i + 1] == d->h_off[i]) {
      if (s->iso_first < 0) s->iso_first = i;
      s->iso_count++;
    }
  s->h_nnz = 9 * d->nnz_coef;
  s->h_row_offsets.resize(3 * (size_t)N + 1);
  s->h_col_indices.resize((size_t)s->h_nnz);
  s->h_row_offsets[0] = 0;
  for (int i = 0; i < N; i++) {
    const int deg = d->h_off[i + 1] - d->h_off[i];
    for (int c = 0; c < 3; c++) s->h_row_offsets[3 * i + c + 1] = s->h_row_offsets[3 * i + c] + 3 * deg;
  }
#pragma omp parallel for schedule(static)
  for (int r = 0; r < 3 * N; r++) {
    const int ci = r / 3;
    int o = s->h_row_offsets[r];
    for (int k = d->h_off[ci]; k < d->h_off[ci + 1]; k++) {
      const int b = 3 * d->h_cols[k];
      s->h_col_indices[o++] = b;
      s->h_col_indices[o++] = b + 1;
      s->h_col_indices[o++] = b + 2;
    }
  }
  TRY(dmalloc(&s->d_H, (size_t)s->h_nnz));
  if (d->kind == kT10 && s->asm_mode != 1 && d->h_X0.size() == 3 * (size_t)N) {
    // row groups of the fused tangent + assembly kernel (the element-block buffer Kbuf is then never allocated
    // unless the material is switched to Mooney-Rivlin: ensure_kbuf): the affine form where it applies, else the general one
    bool affine = false;
    TRY(setup_affine_form(s, &affine));
    if (!affine) TRY(setup_general_form(s));
    s->geom_gen_seen = d->geom_gen;
  }
  s->sparsity_done = true;
  if (s->verbose)
    std::printf("Sparse Hessian: %d x %d, nnz = %d\n", 3 * N, 3 * N, s->h_nnz);
  return 0;
}

// A node of no element (and of no general linear constraint row, which would seed its diagonal) has an empty row in H:
// the element-level results stay defined (zero mass, zero internal force, that empty row), a solve with H does not --
// extract_dinv_kernel would invert the next node's diagonal block for it.  Found on the host by
// tlfea_newton_analyze_hessian_sparsity.  The guard stands at the two places every use of H^-1 or of its diagonal blocks
// goes through -- pcg() (the direct solve included) and stage 0 of precond_setup (solves, the modal iteration, the
// preconditioner test hooks) -- and, so that a step does not launch its gradient and assembly first, at the top of the
// entry points that begin a step.
int tlfea::refuse_empty_rows(tlfea_newton_t s, const char* who) {
  if (s->iso_count == 0) return 0;
  return fail(std::string(who) + ": node " + std::to_string(s->iso_first) + " belongs to no element (" +
              std::to_string(s->iso_count) + " such node" + (s->iso_count > 1 ? "s" : "") +
              " found by tlfea_newton_analyze_hessian_sparsity): its row of H is empty, so a solve with H is not defined; "
              "remove unused nodes from the mesh, or use a solver that never forms H (AdamW, Nesterov)");
}

extern "C" int tlfea_newton_hessian_nnz(tlfea_newton_t s, int* nnz) {
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  *nnz = s->h_nnz;
  return 0;
}
extern "C" int tlfea_newton_retrieve_hessian_csr(tlfea_newton_t s, int* ro, int* ci, double* val) {
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  if (ro) std::copy(s->h_row_offsets.begin(), s->h_row_offsets.end(), ro);
  if (ci) std::copy(s->h_col_indices.begin(), s->h_col_indices.end(), ci);
  if (val) {
    TRY(hessian_current(s));
    HIP_TRY(hipStreamSynchronize(s->stream));
    D2H(val, s->d_H, s->h_nnz);
  }
  return 0;
}
// What the last Newton assembly and solve set-up ran on (DESIGN 3g'): out[0] = 1 the last p-multigrid set-up summed Hc and
// R from the image rows assembled from the element records, 0 from the CSR H; out[1] = assemblies of H since the solver
// was created; out[2] = 1 d_H holds the H of the last assembly.
extern "C" int tlfea_newton_get_setup_form(tlfea_newton_t s, long long* out3) {
  if (!s || !out3) return fail("tlfea_newton_get_setup_form: null argument");
  out3[0] = s->sr.last_form;
  out3[1] = s->sr.n_asm;
  out3[2] = s->sr.h_current ? 1 : 0;
  return 0;
}

// UpdateNodalFixed may have changed the size of the fixed set since the solver was built: the multipliers follow it
// (restarting from zero) before anything indexes them with the new constraint ids.
int tlfea::sync_constraints(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  if (!s->cons_enabled || d->n_constraint == s->n_constraints) return 0;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (s->d_lam) (void)hipFree(s->d_lam);
  s->n_constraints = d->n_constraint;
  TRY(dmalloc(&s->d_lam, (size_t)std::max(1, s->n_constraints)));
  HIP_TRY(hipMemset(s->d_lam, 0, (size_t)std::max(1, s->n_constraints) * sizeof(double)));
  if (!dist_on(s)) {
    s->n_constraints_global = s->n_constraints;
    return 0;
  }
  // multi-GPU: the constraint weights follow the new fixed set, and the ranks re-agree on the global count (every rank
  // reaches this point in the same call: UpdateNodalFixed is a collective operation on a partitioned mesh)
  if (s->d_wc) (void)hipFree(s->d_wc);
  s->d_wc = nullptr;
  if (d->n_constraint > 0) {
    std::vector<double> wc((size_t)d->n_constraint);
    for (int k = 0; k < d->n_constraint; k++) wc[k] = s->h_nw[d->h_fixed[k / 3]];
    TRY(dmalloc(&s->d_wc, wc.size()));
    HIP_TRY(hipMemcpy(s->d_wc, wc.data(), wc.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  double cnt = 0.0;   // boundary sums: every holder counts its rows; overlapping partition: owners only
  for (int k = 0; k < d->n_constraint; k++) cnt += s->halo.on ? s->h_nw[d->h_fixed[k / 3]] : 1.0;
  TRY(allreduce_host(s, s->halo.on ? s->halo.d_red : s->d_ibuf, &cnt, 1));
  s->n_constraints_global = (int)(cnt + 0.5);
  return 0;
}
bool tlfea::pinned_on(tlfea_newton_t s) {
  return s->n_constraints > 0 && s->d->is_constraints_setup && s->d->cons_mode == 1;
}
bool tlfea::lincons_on(tlfea_newton_t s) { return s->n_constraints > 0 && s->d->cons_mode == 2 && s->d->n_constraint > 0; }

// the fused tangent + assembly kernel covers T10 with St.Venant-Kirchhoff (+ Kelvin-Voigt); Mooney-Rivlin and the
// ANCF kinds keep the element-block buffer (tangent_blocks + assemble_rows)
static bool use_direct(tlfea_newton_t s) {
  if (!(s->rg_ok && s->asm_mode != 1 && s->d->kind == kT10)) return false;
  if (s->d->mat.model == kSVK) return s->affine_ok || s->d_rg[0] != nullptr;
  return s->d->mat.model == kMooneyRivlin && s->d_rg[0] != nullptr;   // general-form work lists (ensure_form_for_material)
}
// the affine-element form exists for St.Venant-Kirchhoff; Mooney-Rivlin takes the general form (its own instantiation)
static bool affine_now(tlfea_newton_t s) { return s->affine_ok && s->d->mat.model == kSVK; }
// Mooney-Rivlin on a mesh whose work lists were built for the affine form only: the general form's lists on first use
static int ensure_form_for_material(tlfea_newton_t s) {
  if (s->rg_ok && s->asm_mode != 1 && s->d->kind == kT10 && !affine_now(s) && !s->d_rg[0]) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    const bool keep_affine = s->affine_ok;
    TRY(setup_general_form(s));
    s->affine_ok = keep_affine;
    if (!s->d_rg[0]) s->rg_ok = keep_affine;  // no general lists (odd mesh): Mooney-Rivlin keeps the two-kernel path
  }
  return 0;
}
static double fq_h(tlfea_newton_t s) { return affine_now(s) ? s->prm.time_step : 0.0; }
static int fq_slots(tlfea_newton_t s);
// residual launch of the Newton path (the point records it leaves for the fused assembly follow the assembly's form)
static void launch_residual_newton(tlfea_newton_t s, double* Fq, const MassTerm* mt) {
  tlfea_t10_t d = s->d;
  if (Fq) s->mf.valid = false;  // the records no longer belong to the assembled H (the next assembly claims them)
  launch_residual(s->stream, d->view(), d->mat, s->d_v, d->d_fbuf, nullptr, nullptr, nullptr, nullptr, Fq, mt, fq_h(s),
                  fq_slots(s), d->d_emat);
}
// record slots of the affine assembly: point q0 first, then the points where vertex 0, 1, 2, 3 has L = 1/2
static int fq_slots(tlfea_newton_t s) {
  int w = 0;
  if (affine_now(s)) {
    w |= 0 << (4 * s->av.q0);
    for (int p = 0; p < 4; p++) w |= (p + 1) << (4 * s->av.qv[p]);
  }
  return w;
}
static void fill_mass_shape(tlfea_newton_t s, MassTerm& mt);
// the fused launch itself: H of the point records in d_Fq, by the form of the moment
static void launch_fused_kernel(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  const tlfea_newton_params& p = s->prm;
  const int* fixed = pinned_on(s) ? d->d_fixed_slot : nullptr;
  if (affine_now(s))
    launch_assemble_affine(s->stream, d->view(), d->mat, p.time_step, s->rg4, s->av, s->d_Fq, s->d_cmass,
                           d->d_emat ? 1.0 : (d->mass_rho0 > 0.0 ? d->mass_rho0 : 0.0), fixed, s->d_nw,
                           p.time_step * p.time_step * p.rho, s->d_H, d->d_emat);
  else
    launch_assemble_direct(s->stream, d->view(), d->mat, p.time_step, s->rg, s->d_Fq, d->d_mval, fixed, s->d_nw,
                           p.time_step * p.time_step * p.rho, s->d_H, d->d_emat);
  s->sr.h_current = true;
  s->sr.n_asm++;
}
// The affine assembly claims the point records: the matrix-free passes (and the set-up from the records) apply the H of
// THESE records and scalars, whether or not that H is on the device.
static void claim_records(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  const tlfea_newton_params& p = s->prm;
  const int* fixed = pinned_on(s) ? d->d_fixed_slot : nullptr;
  {
    // The matrix-free product applies THIS H: the same records and the same scalars, kept as they are now.  Terms that
    // the callers add to H after this launch (general linear constraints, obstacle blocks) and per-element materials
    // are not reproduced by the element map: such an H is served by the CSR kernel only.
    auto& f = s->mf;
    const double h = p.time_step;
    f.mc.a = h * d->mat.lambda + d->mat.lamd;
    f.mc.b = h * d->mat.mu + d->mat.eta;
    f.mc.c1 = h * d->mat.mu;
    f.mc.cl = h * d->mat.lambda;
    f.mc.w0 = d->h_qw[s->av.q0];
    f.mc.w1 = d->h_qw[s->av.qv[0]];
    f.mc.rho_inv_h = (d->mass_rho0 > 0.0 ? d->mass_rho0 : 0.0) / h;
    MassTerm mt{};
    fill_mass_shape(s, mt);
    for (int q = 0; q < kNQ; q++) {
      f.mc.mw[q] = d->h_qw[q];
      for (int k = 0; k < kNN; k++) f.mc.Nq[q][k] = mt.Nq[q][k];
    }
    f.fixed = fixed;
    f.penalty = p.time_step * p.time_step * p.rho;
    f.valid = !d->d_emat && !lincons_on(s) && d->obs.n == 0;
    f.gen++;
  }
}
static void launch_fused(tlfea_newton_t s) {
  s->mf.valid = false;
  launch_fused_kernel(s);
  if (affine_now(s)) claim_records(s);
}
int tlfea::hessian_current(tlfea_newton_t s) {
  auto& r = s->sr;
  if (r.h_current) return 0;
  if (!affine_now(s) || !s->mf.valid || r.gen != s->mf.gen)
    return fail("the Hessian of the last Newton iteration was not assembled (its solve was set up from the element records) and "
                "the point records are no longer those of that assembly: assemble again (tlfea_newton_assemble_hessian)");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return fail("the Hessian is not assembled inside a stream capture (whoever reads it must call hessian_current before)");
  launch_fused_kernel(s);  // the same kernel on the same records: the H an eager assembly would have left
  HIP_TRY(hipGetLastError());
  return 0;
}
static int ensure_kbuf(tlfea_newton_t s) {
  if (s->d_Kbuf) return 0;
  tlfea_t10_t d = s->d;
  return dmalloc(&s->d_Kbuf, (size_t)d->E * (d->S * (d->S + 1) / 2) * 9);
}

// T10: the inertia term of grad L element by element in the residual launch (same quadrature rule as the mass matrix,
// the density it was assembled with) instead of the mass CSR product with gathered velocities
static bool mass_in_residual(tlfea_newton_t s) {
  return s->mass_mode == 0 && s->d->kind == kT10 && s->d->mass_rho0 >= 0.0;
}
static int fill_mass_term(tlfea_newton_t s, MassTerm& mt) {
  tlfea_t10_t d = s->d;
  if (!s->d_mbuf) TRY(dmalloc(&s->d_mbuf, (size_t)d->Epad * 6 * d->S));
  mt.vprev = s->d_vprev;
  mt.mbuf = s->d_mbuf;
  mt.rho_inv_h = (d->d_emat ? 1.0 : d->mass_rho0) / s->prm.time_step;  // per-element: x the record's density
  fill_mass_shape(s, mt);
  return 0;
}
// shape functions at the rule's points (the rule of the mass matrix, FEAT10Data.cu:206-278)
void tlfea::shape_at_rule_points(tlfea_t10_t d, double Nq[kNQ][kNN]) {
  const int edges[6][2] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {1, 3}, {2, 3}};  // FEAT10Data.cu:143
  for (int q = 0; q < kNQ; q++) {
    const double L[4] = {1.0 - d->h_q[0][q] - d->h_q[1][q] - d->h_q[2][q], d->h_q[0][q], d->h_q[1][q], d->h_q[2][q]};
    for (int k = 0; k < 4; k++) Nq[q][k] = L[k] * (2.0 * L[k] - 1.0);
    for (int k = 0; k < 6; k++) Nq[q][k + 4] = 4.0 * L[edges[k][0]] * L[edges[k][1]];
  }
}
static void fill_mass_shape(tlfea_newton_t s, MassTerm& mt) { shape_at_rule_points(s->d, mt.Nq); }

// ---- matrix-free product of the CG iteration --------------------------------------------------------------
// TLFEA_SPMV_MATFREE: 0 never, 1 wherever eligible, unset = eligible and at least kMatfreeMinRows node rows
static int matfree_env() {
  static const int m = env_tristate("TLFEA_SPMV_MATFREE");
  return m;
}
// Two launches (plus the direction kernel on meshes that would run the fused SpMV) replace one.  Measured on the SVK bars
// (DESIGN 3g): a tie at 30 k nodes, -12 % per Newton iteration at 172 k, -10 % at 402 k, -13 % at 1.34 M; between 30 k and
// 172 k nothing was measured, so the pick starts just below the smallest size measured to win.
constexpr int kMatfreeMinRows = 150000;
bool tlfea::matfree_eligible(tlfea_newton_t s) {
  return affine_now(s) && s->mf.valid && !dist_on(s) && !lincons_on(s) && s->d->obs.n == 0 && !s->d->d_emat && !s->spmv32_now;
}
bool tlfea::matfree_chosen(tlfea_newton_t s) {
  if (matfree_env() == 0 || !matfree_eligible(s)) return false;
  return matfree_env() == 1 || s->N >= kMatfreeMinRows;
}
// TLFEA_MATFREE_COMPACT: 1 (default) = a wavefront sums its element rows per node before they are stored
// (matfree_compact.h), 0 = one row per (element, local node) in [10][Epad][3].  Read once per process.
bool tlfea::matfree_compact_env() {
  static const bool on = env_flag("TLFEA_MATFREE_COMPACT", true);
  return on;
}
// TLFEA_MATFREE_POINTS: stored points of the packed F records (matfree_records.h) of both real types, 4 = the
// outer points (the centroid's F is their mean), 5 = all.  Unset: the measured choice per type (DESIGN 3g, 3g').  Read once
// per process.
constexpr int kMatfreePoints64 = 5, kMatfreePoints32 = 5;
int tlfea::matfree_points(bool single) {
  static const int forced = env_int("TLFEA_MATFREE_POINTS", 0);
  if (forced == 4 || forced == 5) return forced;
  return single ? kMatfreePoints32 : kMatfreePoints64;
}
// the element rows' buffer (233 MB at config C, 75 MB in the compact form) and the compact form's lists: on first use,
// and outside any stream capture
int tlfea::matfree_ensure_buffer(tlfea_newton_t s) {
  auto& f = s->mf;
  if (f.d_ybuf) return 0;
  tlfea_t10_t d = s->d;
  if (!matfree_compact_env()) return dmalloc(&f.d_ybuf, (size_t)d->Epad * 3 * kNN);
  MatfreeCompactHost h;
  if (!build_matfree_compact(s->N, d->E, d->h_conn.data(), h)) return fail("matrix-free product: malformed connectivity");
  int *d_row_off = nullptr, *d_n2r_off = nullptr, *d_n2r = nullptr;
  unsigned short *d_src = nullptr, *d_desc = nullptr;
  TRY(dmalloc(&d_row_off, h.row_off.size()));
  f.d_cp[0] = d_row_off;
  TRY(dmalloc(&d_src, h.src.size()));
  f.d_cp[1] = d_src;
  TRY(dmalloc(&d_desc, h.desc.size()));
  f.d_cp[2] = d_desc;
  TRY(dmalloc(&d_n2r_off, h.n2r_off.size()));
  f.d_cp[3] = d_n2r_off;
  TRY(dmalloc(&d_n2r, h.n2r.size()));
  f.d_cp[4] = d_n2r;
  HIP_TRY(hipMemcpy(d_row_off, h.row_off.data(), h.row_off.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_src, h.src.data(), h.src.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_desc, h.desc.data(), h.desc.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_n2r_off, h.n2r_off.data(), h.n2r_off.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_n2r, h.n2r.data(), h.n2r.size() * sizeof(int), hipMemcpyHostToDevice));
  f.cp = MatfreeCompact{d_row_off, d_src, d_desc, d_n2r_off, d_n2r};
  f.cp_rows = h.rows();
  f.cp_ratio = h.ratio(d->E);
  f.compact = true;
  return dmalloc(&f.d_ybuf, (size_t)f.cp_rows * 3);
}
// The packed fp64 records the product reads: g once per affine set-up, F once per assembly (mf.gen).  Allocates on first
// use: before the first product of an assembly and outside any stream capture.
int tlfea::matfree_ensure_records(tlfea_newton_t s) {
  auto& f = s->mf;
  tlfea_t10_t d = s->d;
  const int np = matfree_points(false);
  if (!f.d_gp) {
    TRY(dmalloc(&f.d_gp, mfr_g_len((size_t)d->E)));
    TRY(dmalloc(&f.d_Fp, mfr_F_len((size_t)d->E, np)));
    f.gp_ok = false;
    f.rec_gen = -1;
  }
  const bool g = !f.gp_ok, F = f.rec_gen != f.gen;
  if (g || F) launch_matfree_pack<double>(s->stream, d->E, np, F ? s->d_Fq : nullptr, g ? s->d_gvec : nullptr, f.d_Fp, f.d_gp);
  f.gp_ok = true;
  f.rec_gen = f.gen;
  HIP_TRY(hipGetLastError());
  return 0;
}
// q = H p and the p.q slots from the element records (p as pcg_direction_kernel left it)
int tlfea::launch_matfree_product(tlfea_newton_t s, const double* p, double* q, double* pq_part) {
  tlfea_t10_t d = s->d;
  auto& f = s->mf;
  const MatfreeCompact* cp = f.compact ? &f.cp : nullptr;
  if (!f.gp_ok || f.rec_gen != f.gen)
    return fail("matrix-free Hessian product: the packed element records are not those of the assembled H");
  launch_tangent_apply_affine(s->stream, d->view(), matfree_points(false), f.d_gp, f.d_Fp, f.mc, p, f.d_ybuf, cp);
  launch_matfree_gather(s->stream, s->N, d->Epad, d->inc(), f.d_ybuf, p, f.fixed, s->d_nw, f.penalty, q, pq_part, cp);
  return 0;
}

// contact gradient of the rigid obstacles (g may be null: refresh of the per-node force / block buffers only)
static void launch_obstacles_grad(tlfea_newton_t s, double* g) {
  tlfea_t10_t d = s->d;
  if (d->kind != kT10) {  // DESIGN 3e': sample points per element, then the coefficient-owner gather
    launch_ancf_obstacle_points(s->stream, ancf_obs_view(d), d->obs, d->d_x, d->d_y, d->d_z, s->d_xp, s->d_yp, s->d_zp,
                                s->prm.time_step);
    launch_ancf_obstacle_gather(s->stream, s->N, d->inc(), d->d_ao_cbuf, d->d_ao_fc, g);
    return;
  }
  launch_obstacle_grad(s->stream, (int)d->h_surf.size(), d->d_ob_node, d->d_ob_w, d->obs, d->d_x, d->d_y, d->d_z, s->d_xp,
                       s->d_yp, s->d_zp, s->prm.time_step, pinned_on(s) ? d->d_fixed_slot : nullptr, g, d->d_ob_f,
                       d->d_ob_blk, d->d_ob_fk);
}
// + h x the contact blocks on the diagonal of H: after the assembly and the constraint term, before anything reads H
static void launch_obstacles_hessian(tlfea_newton_t s, bool buffers_fresh) {
  tlfea_t10_t d = s->d;
  if (d->obs.n == 0 || d->kind != kT10) return;  // ANCF: in Kbuf before the row assembly (launch_ancf_obstacles_tangent)
  if (!buffers_fresh) launch_obstacles_grad(s, nullptr);
  launch_obstacle_hessian(s->stream, (int)d->h_surf.size(), d->d_ob_node, d->d_off, d->d_diagpos, d->d_ob_blk,
                          s->prm.time_step, s->d_H);
}

// ANCF: + h sum_p S_i S_j C_p on the element blocks of every touched element, between the element tangent and the rows
static void launch_ancf_obstacles_tangent(tlfea_newton_t s, bool buffers_fresh) {
  tlfea_t10_t d = s->d;
  if (d->obs.n == 0 || d->kind == kT10) return;
  if (!buffers_fresh) launch_obstacles_grad(s, nullptr);
  launch_ancf_obstacle_tangent(s->stream, ancf_obs_view(d), s->prm.time_step, s->d_Kbuf);
}

static AncfLoadView ancf_load_view(tlfea_t10_t h) {
  return AncfLoadView{h->E, h->S, h->d_conn, h->d_ld_cls, h->d_ld_tab, h->d_ld_qw, h->d_ld_mask, h->d_ld_pe, h->d_ld_lbuf};
}
static T10LoadView t10_load_view(tlfea_t10_t h) {
  return T10LoadView{(int)h->h_ld_lf.size(), h->d_ld_fnodes, h->d_ld_pe, h->d_ld_lbuf};
}
// g -= f_load(x): the constant part is rebuilt when the mass matrix, the acceleration or a traction changed;
// the pressure rows follow the current coefficients
static int launch_loads_grad(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  const bool has_const = d->ld_have_a || d->ld_n_trac > 0;
  if (has_const && d->ld_const_dirty) {
    if (d->ld_have_a && !mass_assembled(d))
      return fail("a body acceleration is set but the mass matrix was dropped: CalcMassMatrix must run again");
    launch_body_force(s->stream, s->N, d->inc(), d->ld_have_a ? d->d_mval : nullptr, d->kind == kT10 ? 1 : 4, d->ld_a,
                      d->ld_n_trac > 0 ? d->d_ld_tr : nullptr, d->d_ld_fc);
    d->ld_const_dirty = false;
  }
  Incidence inc = d->inc();
  if (d->ld_n_press > 0 && d->kind == kT10) {  // rows of the loaded boundary faces, through their own node-to-row CSR
    launch_t10_pressure(s->stream, t10_load_view(d), d->d_x, d->d_y, d->d_z);
    inc.n2e_off = d->d_ld_foff;
    inc.n2e = d->d_ld_fslot;
  } else if (d->ld_n_press > 0) {
    launch_ancf_pressure(s->stream, ancf_load_view(d), d->d_x, d->d_y, d->d_z);
  }
  launch_load_gather(s->stream, s->N, inc, has_const ? d->d_ld_fc : nullptr,
                     d->ld_n_press > 0 ? d->d_ld_lbuf : nullptr, d->d_ld_f, s->d_g);
  return 0;
}

static int eval_gradient(tlfea_newton_t s, double* norm_g) {
  tlfea_t10_t d = s->d;
  if (d->obs.n > 0 && dist_on(s))  // before any collective
    return fail("rigid obstacles are not supported on the partitioned path (clear them first)");
  if (d->loads_on() && dist_on(s))
    return fail("distributed loads are not supported on the partitioned path (clear them first)");
  TRY(refresh_geometry(s));
  TRY(ensure_form_for_material(s));
  const tlfea_newton_params& p = s->prm;
  const bool mir = mass_in_residual(s);
  {
    StageTimer t(s, 0);
    MassTerm mt{};
    if (mir) TRY(fill_mass_term(s, mt));
    launch_residual_newton(s, (use_direct(s) && s->fq_in_residual) ? s->d_Fq : nullptr, mir ? &mt : nullptr);
    d->fbuf_valid = !mir;
    t.stop();
  }
  {
    StageTimer t(s, 1);
    const bool pinned = pinned_on(s);
    if (mir)
      launch_grad_light(s->stream, s->N, d->Epad, d->inc(), d->d_fbuf, s->d_mbuf, d->d_fext, d->d_x, d->d_y, d->d_z, d->d_xt,
                        d->d_yt, d->d_zt, pinned ? d->d_fixed_slot : nullptr, s->d_lam, s->d_nw, p.time_step, p.rho,
                        d->d_fint, d->d_cons, s->d_g);
    else
    launch_grad(s->stream, s->N, d->inc(), d->d_fbuf, d->d_mval, s->d_v, s->d_vprev, d->d_fext, d->d_x, d->d_y, d->d_z,
                d->d_xt, d->d_yt, d->d_zt, pinned ? d->d_fixed_slot : nullptr, s->d_lam, s->d_nw, p.time_step, p.rho,
                d->d_fint, d->d_cons, s->d_g);
    if (lincons_on(s)) {
      // general linear rows: c = J x - rhs, then g += h J^T (lambda + rho c)   (SyncedNewton.cu:377-404)
      launch_lin_constraint(s->stream, d->n_constraint, d->d_joff, d->d_jcol, d->d_jval, d->d_rhs, d->d_x, d->d_y, d->d_z,
                            d->d_cons);
      launch_lin_constraint_grad(s->stream, 3 * s->N, d->d_jtoff, d->d_jtcol, d->d_jtval, s->d_lam, d->d_cons,
                                 p.time_step, p.rho, s->d_g);
    }
    if (d->obs.n > 0) launch_obstacles_grad(s, s->d_g);
    if (d->loads_on()) TRY(launch_loads_grad(s));
    HIP_TRY(hipGetLastError());
    // each rank's g holds only its own elements' forces and its share of M, f_ext, constraints on
    // partition-boundary nodes: sum the boundary entries over ranks (nothing else is exchanged)
    TRY(iface_sum(s, s->d_g, 3));
    if (norm_g) TRY(device_norm(s, s->d_g, s->d_w, 3 * s->N, norm_g));  // first-order solvers test only now and then
    t.stop();
  }
  return 0;
}

// fq_fresh: the per-point F buffer holds the F of the CURRENT coordinates (true right after eval_gradient, which is
// how the Newton loop calls it); a stand-alone assembly refreshes it with a residual launch first
int tlfea::assemble(tlfea_newton_t s, bool fq_fresh, bool lazy) {
  tlfea_t10_t d = s->d;
  const bool after_grad = fq_fresh;  // the obstacle buffers hold the current coordinates' blocks
  {
    const long seen = s->geom_gen_seen;
    TRY(refresh_geometry(s));
    if (seen != s->geom_gen_seen) fq_fresh = false;  // the point records follow the assembly's form: rewrite them
    const bool had_general = s->d_rg[0] != nullptr;
    TRY(ensure_form_for_material(s));
    if (!had_general && s->d_rg[0]) fq_fresh = false;
  }
  const tlfea_newton_params& p = s->prm;
  const bool pinned = pinned_on(s);
  if (use_direct(s)) {
    StageTimer t(s, 3);
    if (!fq_fresh)
      launch_residual_newton(s, s->d_Fq, nullptr);
    // The Newton loop's assembly, where nothing of the solve would read the CSR H (DESIGN 3g'): the records are claimed as
    // the assembly claims them, and the image rows of R and the fine block diagonal are written in H's place.  Whoever
    // needs H after all gets it from hessian_current().
    if (lazy && affine_now(s)) {
      s->mf.valid = false;
      claim_records(s);
      bool rec = false;
      TRY(setup_records_decide(s, &rec));
      if (rec) {
        s->sr.h_current = false;
        TRY(setup_records_assemble(s));
        HIP_TRY(hipGetLastError());
        t.stop();
        return 0;
      }
      launch_fused_kernel(s);
    } else
      launch_fused(s);
    if (lincons_on(s))  // + h^2 rho J^T J  (SyncedNewton.cu:292-341)
      launch_lin_constraint_hessian(s->stream, 3 * s->N, d->d_jtoff, d->d_jtcol, d->d_jtval, d->d_joff, d->d_jcol,
                                    d->d_jval, d->d_off, d->d_cols, p.time_step * p.time_step * p.rho, s->d_H);
    launch_obstacles_hessian(s, after_grad);
    HIP_TRY(hipGetLastError());
    t.stop();
    return 0;
  }
  TRY(ensure_kbuf(s));
  {
    StageTimer t(s, 2);
    launch_tangent_blocks(s->stream, d->view(), d->mat, p.time_step, s->d_Kbuf, d->d_emat);
    t.stop();
  }
  {
    StageTimer t(s, 3);
    launch_ancf_obstacles_tangent(s, after_grad);
    launch_assemble_rows(s->stream, s->N, d->S, d->maxdeg, d->inc(), s->d_Kbuf, d->d_mval, 1.0 / p.time_step,
                         pinned ? d->d_fixed_slot : nullptr, s->d_nw, p.time_step * p.time_step * p.rho, s->d_H);
    s->sr.h_current = true;
    s->sr.n_asm++;
    if (lincons_on(s))  // + h^2 rho J^T J  (SyncedNewton.cu:292-341)
      launch_lin_constraint_hessian(s->stream, 3 * s->N, d->d_jtoff, d->d_jtcol, d->d_jtval, d->d_joff, d->d_jcol,
                                    d->d_jval, d->d_off, d->d_cols, p.time_step * p.time_step * p.rho, s->d_H);
    launch_obstacles_hessian(s, after_grad);
    HIP_TRY(hipGetLastError());
    t.stop();
  }
  return 0;
}

extern "C" int tlfea_newton_get_assembly_mode(tlfea_newton_t s) {
  if (!s) return 0;
  if (tlfea_newton_analyze_hessian_sparsity(s)) return 0;
  if (ensure_form_for_material(s)) return 0;
  return (use_direct(s) && (affine_now(s) || s->d_rg[0])) ? (affine_now(s) ? 3 : 2) : 1;
}
extern "C" int tlfea_newton_get_assembly_form(tlfea_newton_t s, int* out8) {
  if (!s || !out8) return fail("tlfea_newton_get_assembly_form: null argument");
  std::fill(out8, out8 + 8, 0);
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  TRY(ensure_form_for_material(s));
  tlfea_t10_t d = s->d;
  const bool pe = d->d_emat != nullptr;
  const int mode = tlfea_newton_get_assembly_mode(s);
  out8[0] = mode;
  if (mode == 3) {
    const AssemblyLaunchForm f = assemble_affine_form(s->rg4, pe);
    out8[1] = 1;
    out8[3] = s->rg4.G;
    out8[4] = s->rg4.acc_max;
    out8[5] = (int)f.lds;
    out8[6] = f.grid;
    out8[7] = s->rg4_passes;
  } else if (mode == 2) {
    const AssemblyLaunchForm f = assemble_direct_form(s->rg, d->mat, pe);
    out8[1] = f.rolled;
    out8[3] = s->rg.G;
    out8[4] = s->rg.acc_max;
    out8[5] = (int)f.lds;
    out8[6] = f.grid;
    out8[7] = s->rg_passes;
  } else {  // tangent blocks + one workgroup per node row
    out8[1] = 1;
    out8[2] = tangent_blocks_wpb(pe && d->S == 10);
    out8[3] = s->N;
    out8[4] = 9 * d->maxdeg;
    out8[5] = (int)assemble_rows_lds(d->maxdeg);
    out8[6] = s->N;
    out8[7] = 1;
  }
  return 0;
}
extern "C" int tlfea_newton_get_gradient_form(tlfea_newton_t s) {
  if (!s) return 0;
  return mass_in_residual(s) ? 2 : 1;
}
extern "C" int tlfea_newton_eval_gradient(tlfea_newton_t s, double* norm_g) {
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  TRY(sync_constraints(s));
  return eval_gradient(s, norm_g);
}
extern "C" int tlfea_newton_assemble_hessian(tlfea_newton_t s) {
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  TRY(assemble(s, /*fq_fresh=*/false));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return 0;
}

// Average duration (ms) of each hot kernel over `reps` back-to-back launches on the launch stream, bracketed by
// one hipEvent pair per kernel (no host work between launches, so the figure is kernel time + the ~1.5 us
// same-stream boundary, directly comparable with rocprofv3 --kernel-trace).  The launches recompute what the
// last Newton iteration computed (same inputs, same outputs), so the solver state is unchanged.
// out[0] residual, [1] tangent blocks, [2] row assembly, [3] CG SpMV, [4] Chebyshev step (SpMV + vector updates).
extern "C" int tlfea_newton_time_kernels(tlfea_newton_t s, int reps, double* out_ms4) {  // out: 6 entries
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  // the CSR launches below read H: where the last Newton iteration left it unassembled and its records have moved since,
  // a measurement takes the H of the current coordinates
  if (!s->sr.h_current && hessian_current(s)) TRY(assemble(s, /*fq_fresh=*/false));
  tlfea_t10_t d = s->d;
  const tlfea_newton_params& p = s->prm;
  if (reps < 1) reps = 1;
  const int N = s->N;
  const bool fused = s->pcg_fused < 0 ? (N <= 200000) : (s->pcg_fused != 0);
  out_ms4[5] = out_ms4[6] = 0.0;
  // cheb_step and the cycle pattern price the stream of the stored copy, whichever form the last set-up's smoother took
  TRY(ensure_fine_copy(s));
  // geo -1: a measurement is no solve, the geometry read-back keeps the solver's last launch
  C32Level Lf = fine_c32(s);
  Lf.geo = -1;
  const PolyLevel& V = s->pmg.vertex;
  const C32Level Lc = V.c32(cheb_bits_eff(s), -1);
  for (int k = 0; k < 7; k++) {
    if (k >= 5 && !(s->pmg.ok && s->pmg.vertex.d_B8)) break;
    auto launch = [&](int r) -> int {  // one repetition of kernel k
      if (k == 0) {
        MassTerm mt{};
        const bool mir = mass_in_residual(s);
        if (mir) TRY(fill_mass_term(s, mt));
        launch_residual_newton(s, use_direct(s) ? s->d_Fq : nullptr, mir ? &mt : nullptr);
      }
      else if (k == 1) {
        if (use_direct(s)) return kStopReps;  // no separate tangent launch on the fused path: out[1] = 0
        TRY(ensure_kbuf(s));
        launch_tangent_blocks(s->stream, d->view(), d->mat, p.time_step, s->d_Kbuf, d->d_emat);
      } else if (k == 2 && use_direct(s))  // out[2] = the fused tangent + assembly launch
        launch_fused(s);
      else if (k == 2)
        launch_assemble_rows(s->stream, N, d->S, d->maxdeg, d->inc(), s->d_Kbuf, d->d_mval, 1.0 / p.time_step,
                             pinned_on(s) ? d->d_fixed_slot : nullptr, s->d_nw,
                             p.time_step * p.time_step * p.rho, s->d_H);
      else if (k == 3)  // the CG iteration's launch (beta from the reduction slots as in the solver; p ping-pongs)
        launch_spmv_dir_dot(s->stream, N, d->inc(), s->d_H, s->d_zv, (r & 1) ? s->d_p2 : s->d_p, 0, part(s, 1), part(s, 0),
                            fused ? ((r & 1) ? s->d_p : s->d_p2) : ((r & 1) ? s->d_p2 : s->d_p), s->d_q, part(s, 2), fused,
                            s->spmv_nt);
      else if (k == 6) {
        // the polynomial-step kernel in the order of one V-cycle: fine, fine, kc-1 coarse, fine (the cycle's last fine
        // step is another instantiation).  Both levels run the SAME kernel, so this is the per-launch average that
        // rocprofv3 reports under the kernel's name (the levels evict each other's matrix from L2 between launches).
        C32Vecs f(s->d_f32, 3 * (size_t)N), c(V.d_f32, 3 * (size_t)V.N);
        const int kc = pmg_coarse_degree_eff(s);
        const double* cf = s->pmg.d_coef;
        c32_step(s, Lf, f, N, cf + 2, s->d_r, s->d_zv, part(s, 0), false);
        c32_step(s, Lf, f, N, cf + 2, s->d_r, s->d_zv, part(s, 0), false);
        c.swap();  // as after the cycle's restriction: the first vertex-level step reads the second buffers
        const double* cc = cf + pmg_table(s).coarse() + 2;
        for (int j = 1; j < kc; j++) c32_step(s, Lc, c, V.N, cc, s->d_r, s->d_zv, part(s, 0), false);
        c32_step(s, Lf, f, N, cf + 2, s->d_r, s->d_zv, part(s, 0), false);
      } else if (k == 5) {  // one step of the coarse-level polynomial of the p-multigrid cycle
        C32Vecs c(V.d_f32, 3 * (size_t)V.N);
        if (r & 1) c.swap();  // each step reads what the last one wrote
        c32_step(s, Lc, c, V.N, s->pmg.d_coef + pmg_table(s).coarse() + 2, s->d_r, s->d_zv, part(s, 0), false);
      } else if (cheb_bits_eff(s) != 64 && s->d_B8 && !s->ar) {  // one step of the polynomial, buffers ping-pong as in
        C32Vecs f(s->d_f32, 3 * (size_t)N);                      // cheb_apply (each step reads what the last one wrote)
        if (r & 1) f.swap();
        c32_step(s, Lf, f, N, s->d_coef + 2, s->d_r, s->d_zv, part(s, 0), false);
      } else if (cheb_bits_eff(s) != 64 && s->d_B8)
        launch_cheb_lp(s->stream, N, d->nnz_coef, d->inc(), s->d_B8, s->d_B1, cheb_bits_eff(s), s->d_Dinv_s, s->d_sc,
                       s->d_cd, s->d_coef + 2, s->d_cd2, s->d_cz, s->d_cz2, s->d_cres, s->d_cres2, s->d_r, s->d_w, part(s, 0), 0);
      else  // fp64 polynomial step
        launch_cheb_step(s->stream, N, d->inc(), s->d_H, s->d_Dinv, s->d_cd, s->d_coef + 2, s->d_cd2, s->d_zv, s->d_cres,
                         s->d_r, s->d_w, part(s, 0), false);
      return 0;
    };
    TRY(time_reps(s->stream, reps, &out_ms4[k], launch));
    if (k == 6) out_ms4[k] /= (double)(pmg_coarse_degree_eff(s) + 2);  // per launch of the cycle pattern
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
extern "C" int tlfea_newton_get_matfree_rows(tlfea_newton_t s, long long* rows, double* ratio) {
  if (!s || !s->mf.d_ybuf) return -1;
  if (rows) *rows = s->mf.compact ? s->mf.cp_rows : (long long)kNN * s->d->E;
  if (ratio) *ratio = s->mf.compact ? s->mf.cp_ratio : 1.0;
  return s->mf.compact ? 1 : 0;
}
// Test hook: the element records of the matrix-free passes.  which 0 / 1 = the element-major g [E][16] / F [E][5][10] in
// fp64, 2 / 3 = the packed g / F (matfree_records.h) of the fp64 product (single = 0) or of the float smoother passes.
// len = values of that buffer; out may be null (length only); points = stored points of the packed F of that type.
extern "C" int tlfea_newton_get_matfree_records(tlfea_newton_t s, int single, int which, void* out, long long* len,
                                                int* points) {
  if (!s || which < 0 || which > 3) return fail("tlfea_newton_get_matfree_records: bad argument");
  if (!s->d_gvec || !s->d_Fq || !s->mf.valid)
    return fail("tlfea_newton_get_matfree_records: no element records of an assembled H (affine T10 form only)");
  const size_t E = (size_t)s->d->E;
  const int np = matfree_points(single != 0);
  const void* src = nullptr;
  size_t n = 0, width = which < 2 || !single ? sizeof(double) : sizeof(float);
  if (which == 0) src = s->d_gvec, n = E * 16;
  else if (which == 1) src = s->d_Fq, n = E * 50;
  else if (single) {
    if (!fine_matfree_live(s)) return fail("tlfea_newton_get_matfree_records: no float records of the assembled H");
    src = which == 2 ? s->fmf.d_g32 : s->fmf.d_F32;
    n = which == 2 ? mfr_g_len(E) : mfr_F_len(E, np);
  } else {
    if (!s->mf.d_gp || !s->mf.gp_ok || s->mf.rec_gen != s->mf.gen)
      return fail("tlfea_newton_get_matfree_records: no packed fp64 records of the assembled H");
    src = which == 2 ? s->mf.d_gp : s->mf.d_Fp;
    n = which == 2 ? mfr_g_len(E) : mfr_F_len(E, np);
  }
  if (len) *len = (long long)n;
  if (out) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(out, src, n * width, hipMemcpyDeviceToHost));
  }
  if (points) *points = np;
  return 0;
}

static int newton_update(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  StageTimer t(s, 5);
  // overlapping partition: the solve leaves dv exact on the owned nodes (and a few ghost layers); every ghost a rank
  // holds moves with its owner's value
  TRY(halo_refresh_f64(s, 0, s->halo.depth, 3, s->d_dv));
  launch_newton_update(s->stream, s->N, s->d_dv, s->d_v, s->d_xp, s->d_yp, s->d_zp, s->prm.time_step, d->d_x, d->d_y,
                       d->d_z);
  t.stop();
  return 0;
}

static int begin_step(tlfea_newton_t s) {  // cudss_solve_update_pos_prev (SyncedNewton.cu:413-422)
  tlfea_t10_t d = s->d;
  const size_t nb = (size_t)s->N * sizeof(double);
  HIP_TRY(hipMemcpyAsync(s->d_xp, d->d_x, nb, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->d_yp, d->d_y, nb, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->d_zp, d->d_z, nb, hipMemcpyDeviceToDevice, s->stream));
  return 0;
}

extern "C" int tlfea_newton_iteration(tlfea_newton_t s, double* norm_g, int* iters) {
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  TRY(refuse_empty_rows(s, "tlfea_newton_iteration"));
  TRY(sync_constraints(s));
  s->lin_worst_rel = 0.0;
  s->lin_all_ok = true;
  double ng = 0.0;
  TRY(eval_gradient(s, &ng));
  launch_axpy_neg(s->stream, 3 * s->N, s->d_g, s->d_b);  // b = -g
  TRY(assemble(s, true, true));
  int it = 0;
  TRY(pcg(s, s->d_b, s->d_dv, &it, nullptr));
  TRY(newton_update(s));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (norm_g) *norm_g = ng;
  if (iters) *iters = it;
  return 0;
}

// One implicit step: SyncedNewtonSolver::OneStepNewtonCuDSS, T10 branch (SyncedNewton.cu:1032-1146)
extern "C" int tlfea_newton_solve(tlfea_newton_t s) {
  if (!s) return fail("null handle");
  tlfea_t10_t d = s->d;
  if (!d->have_dndu) return fail("CalcDnDuPre must be called before Solve");
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  TRY(refuse_empty_rows(s, "tlfea_newton_solve"));
  TRY(sync_constraints(s));
  s->lin_worst_rel = 0.0;
  s->lin_all_ok = true;
  const tlfea_newton_params& p = s->prm;
  const int n = 3 * s->N;
  hipEvent_t e0 = s->ev[2], e1 = s->ev[3];
  HIP_TRY(hipEventRecord(e0, s->stream));
  // state at the start of the step: a linear solve that fails in a LATER Newton iteration must not leave the step half
  // advanced (v, x moved by the earlier iterations, v_prev / lambda by earlier outer iterations)
  if (!s->d_step0) TRY(dmalloc(&s->d_step0, 2 * (size_t)n));
  if (s->n_constraints > s->lam0_cap) {
    if (s->d_lam0) (void)hipFree(s->d_lam0);
    s->d_lam0 = nullptr;
    TRY(dmalloc(&s->d_lam0, (size_t)s->n_constraints));
    s->lam0_cap = s->n_constraints;
  }
  HIP_TRY(hipMemcpyAsync(s->d_step0, s->d_v, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->d_step0 + n, s->d_vprev, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  if (s->n_constraints > 0)
    HIP_TRY(hipMemcpyAsync(s->d_lam0, s->d_lam, (size_t)s->n_constraints * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  TRY(begin_step(s));
  int n_outer = 0, n_newton = 0, pcg_total = 0;
  double norm_g = 0.0, norm_c = 0.0;
  const int fail_hook = env_int("TLFEA_TEST_FAIL_LINSOLVE", -1);
  // Rigid obstacles with friction: the regularised Coulomb term switches between a stiff stick branch and a sliding branch
  // whose exact Hessian has no stiffness along the slip, so a full Newton step can jump across the stick window and back
  // forever.  The step is then halved (up to kMaxHalvings times) until ||g|| decreases; the gradient of the
  // accepted point is the next iteration's.  Without friction nothing of this runs.
  bool friction_on = false;
  for (int k = 0; k < d->obs.n; k++) friction_on = friction_on || d->obs.o[k].mu > 0.0;
  const int kMaxHalvings = 8;
  bool inner_met = false;  // the last outer iteration's Newton loop left through its tolerance test
  auto run = [&]() -> int {
    for (int outer = 0; outer < p.max_outer; ++outer) {
      n_outer++;
      inner_met = false;
      double norm_g0 = -1.0;
      bool g_current = false;
      for (int it = 0; it < p.max_inner; ++it) {
        if (!g_current) TRY(eval_gradient(s, &norm_g));
        g_current = false;
        if (s->verbose) std::printf("  outer %d newton %d ||g|| = %.6e\n", outer, it, norm_g);
        if (norm_g0 < 0.0) norm_g0 = norm_g;
        if (norm_g < p.inner_atol || (p.inner_rtol > 0.0 && norm_g0 > 0.0 && norm_g <= p.inner_rtol * norm_g0)) {
          inner_met = true;
          break;
        }
        launch_axpy_neg(s->stream, n, s->d_g, s->d_b);                       // r = -g  (:494-502)
        TRY(assemble(s, true, true));                                                    // (:1080-1097)
        int iters = 0;
        int rc = pcg(s, s->d_b, s->d_dv, &iters, nullptr);                   // cuDSS factor+solve (:1103-1114)
        pcg_total += iters;
        // TLFEA_TEST_FAIL_LINSOLVE=k (tests only, like TLFEA_CHEB_LMAX_SCALE): the k-th linear solve of the step (0-based)
        // is reported as failed after it ran, to exercise the roll-back of a step that fails in a LATER Newton iteration
        if (!rc && fail_hook >= 0 && n_newton == fail_hook) rc = fail("linear solve failed (TLFEA_TEST_FAIL_LINSOLVE test hook)");
        if (rc) return rc;
        n_newton++;
        TRY(newton_update(s));                                               // v += dv ; x = x_prev + h v (:1116-1119)
        if (friction_on) {
          const double ng_prev = norm_g;
          for (int k = 0;; k++) {
            TRY(eval_gradient(s, &norm_g));
            if (norm_g <= ng_prev || k == kMaxHalvings) break;
            launch_scale(s->stream, n, k == 0 ? -0.5 : 0.5, s->d_dv);  // v = v0 + dv0 / 2^(k+1)
            TRY(newton_update(s));
          }
          g_current = true;
        }
      }
      HIP_TRY(hipMemcpyAsync(s->d_vprev, s->d_v, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice,
                             s->stream));                                    // every OUTER iteration (:1122)
      if (s->n_constraints_global > 0) {
        if (d->cons_mode == 2)
          launch_lin_constraint(s->stream, d->n_constraint, d->d_joff, d->d_jcol, d->d_jval, d->d_rhs, d->d_x, d->d_y,
                                d->d_z, d->d_cons);
        else
          launch_constraint(s->stream, d->n_fixed, d->d_fixed, d->d_x, d->d_y, d->d_z, d->d_xt, d->d_yt, d->d_zt,
                            d->d_cons);
        launch_dual_update(s->stream, s->n_constraints, d->d_cons, p.rho, s->d_lam);  // lambda += rho c (:470-481)
        TRY(device_norm(s, d->d_cons, s->d_wc, s->n_constraints, &norm_c));  // replicated rows weigh 1/multiplicity
        if (s->verbose) std::printf("  outer %d ||c|| = %.6e\n", outer, norm_c);
        if (norm_c < p.outer_tol) break;
      }
    }
    return 0;
  };
  const int rc_step = run();
  if (rc_step) {
    // put the state back to the start of the step (x = x_prev, v, v_prev, lambda as they came in) and report what ran
    const std::string why = api_error();
    const size_t nb = (size_t)s->N * sizeof(double);
    (void)hipMemcpyAsync(s->d_v, s->d_step0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream);
    (void)hipMemcpyAsync(s->d_vprev, s->d_step0 + n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream);
    if (s->n_constraints > 0)
      (void)hipMemcpyAsync(s->d_lam, s->d_lam0, (size_t)s->n_constraints * sizeof(double), hipMemcpyDeviceToDevice, s->stream);
    (void)hipMemcpyAsync(d->d_x, s->d_xp, nb, hipMemcpyDeviceToDevice, s->stream);
    (void)hipMemcpyAsync(d->d_y, s->d_yp, nb, hipMemcpyDeviceToDevice, s->stream);
    (void)hipMemcpyAsync(d->d_z, s->d_zp, nb, hipMemcpyDeviceToDevice, s->stream);
    (void)hipStreamSynchronize(s->stream);
    s->stats[0] = n_outer; s->stats[1] = n_newton; s->stats[2] = norm_g; s->stats[3] = norm_c;
    s->stats[4] = pcg_total; s->stats[5] = 0.0;
    s->adj_state = 3;
    api_error() = why;
    return rc_step;
  }
  HIP_TRY(hipEventRecord(e1, s->stream));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  s->stats[0] = n_outer; s->stats[1] = n_newton; s->stats[2] = norm_g; s->stats[3] = norm_c;
  s->stats[4] = pcg_total; s->stats[5] = ms;
  s->adj_state = n_outer > 1 ? 2 : (inner_met ? 1 : 4);
  if (s->verbose) std::printf("OneStepNewton kernel time: %.3f ms\n", ms);
  return 0;
}

extern "C" int tlfea_newton_retrieve_gradient(tlfea_newton_t s, double* g) { D2H(g, s->d_g, 3 * (size_t)s->N); return 0; }
extern "C" int tlfea_newton_retrieve_velocity(tlfea_newton_t s, double* v) { D2H(v, s->d_v, 3 * (size_t)s->N); return 0; }
extern "C" int tlfea_newton_set_velocity(tlfea_newton_t s, const double* v, const double* v_prev) {
  const size_t nb = 3 * (size_t)s->N * sizeof(double);
  HIP_TRY(hipMemcpy(s->d_v, v, nb, hipMemcpyHostToDevice));
  if (v_prev) HIP_TRY(hipMemcpy(s->d_vprev, v_prev, nb, hipMemcpyHostToDevice));
  return 0;
}
extern "C" int tlfea_newton_set_lambda(tlfea_newton_t s, const double* lam) {
  if (s->n_constraints) HIP_TRY(hipMemcpy(s->d_lam, lam, (size_t)s->n_constraints * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}
extern "C" int tlfea_newton_retrieve_lambda(tlfea_newton_t s, double* lam) {
  if (s->n_constraints) D2H(lam, s->d_lam, (size_t)s->n_constraints);
  return 0;
}
extern "C" int tlfea_newton_get_stats(tlfea_newton_t s, double* st) {
  std::copy(s->stats, s->stats + 6, st);
  return 0;
}
extern "C" int tlfea_newton_n_constraints(tlfea_newton_t s) { return s ? s->n_constraints : -1; }
extern "C" int tlfea_newton_get_stage_ms(tlfea_newton_t s, double* ms, double* counts, int reset) {
  std::copy(s->stage_ms, s->stage_ms + 8, ms);
  if (counts) std::copy(s->stage_n, s->stage_n + 8, counts);
  if (reset) {
    std::fill(s->stage_ms, s->stage_ms + 8, 0.0);
    std::fill(s->stage_n, s->stage_n + 8, 0.0);
  }
  return 0;
}
// Start of an implicit step outside Solve(): x_prev <- x (SyncedNewton.cu:1035) and v_prev <- v (:1122)
extern "C" int tlfea_newton_begin_step(tlfea_newton_t s) {
  TRY(begin_step(s));
  HIP_TRY(hipMemcpyAsync(s->d_vprev, s->d_v, 3 * (size_t)s->N * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  return 0;
}


// What the three handles share: the Newton core whose gradient evaluation they loop around, the six stats words of the
// last Solve (outer iterations, inner iterations or sweeps, ||g||, ||c||, inner flag, ms) and the verbosity.
struct FirstOrder {
  tlfea_newton_t core = nullptr;
  double stats[6] = {0, 0, 0, 0, 0, 0};
  int verbose = 0;
};
// the handle with its core; no solver here assembles, so the core's residual skips the Fq by-product
// (null: refused, the message is set)
template <typename H>
static H* fo_create(const char* who, tlfea_t10_t data, int n_constraints, const void* out) {
  if (!data || !out) return fail(std::string(who) + ": null argument"), nullptr;
  H* a = new H();
  if (tlfea_newton_create(data, n_constraints, &a->core)) return nullptr;
  a->core->fq_in_residual = false;
  return a;
}
template <typename H>
static int fo_destroy(H* a, std::initializer_list<void*> buffers) {
  for (void* p : buffers)
    if (p) (void)hipFree(p);
  (void)tlfea_newton_destroy(a->core);
  delete a;
  return 0;
}
// the reference's SetParameters also clears v_guess, v_prev and lambda (SyncedAdamWNocoop.cuh:175-177,
// SyncedNesterov.cuh:135-137, SyncedVBD.cuh:258-260)
static int fo_clear_state(FirstOrder* a) {
  tlfea_newton_t s = a->core;
  const size_t n = 3 * (size_t)s->N;
  HIP_TRY(hipMemset(s->d_v, 0, n * sizeof(double)));
  HIP_TRY(hipMemset(s->d_vprev, 0, n * sizeof(double)));
  HIP_TRY(hipMemset(s->d_lam, 0, (size_t)std::max(1, s->n_constraints) * sizeof(double)));
  return 0;
}
// Head of a Solve: the core evaluates grad L with ITS parameters, so it takes the time step and rho of this solver; the
// timed span opens; x_prev = x.  Tail: the span closes and the stats words are written.
static int fo_begin(FirstOrder* a, double time_step, double rho) {
  tlfea_newton_t s = a->core;
  s->prm.time_step = time_step;
  s->prm.rho = rho;
  HIP_TRY(hipEventRecord(s->ev[2], s->stream));
  return begin_step(s);
}
static int fo_end(FirstOrder* a, int n_outer, int n_inner, double norm_g, double norm_c, int inner_flag) {
  tlfea_newton_t s = a->core;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[3], s->stream));
  HIP_TRY(hipEventSynchronize(s->ev[3]));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, s->ev[2], s->ev[3]));
  a->stats[0] = n_outer; a->stats[1] = n_inner; a->stats[2] = norm_g; a->stats[3] = norm_c;
  a->stats[4] = inner_flag; a->stats[5] = ms;
  return 0;
}
// what the pass-through entry points of the three solvers call
static int fo_set_verbose(FirstOrder* a, int v) {
  a->verbose = v;
  return 0;
}
static int fo_get_stats(const FirstOrder* a, double* out6) {
  std::copy(a->stats, a->stats + 6, out6);
  return 0;
}

// =================================================================================================
// SyncedAdamWNocoopSolver (SyncedAdamWNocoop.cuh:22-198, SyncedAdamWNocoop.cu:262-500): first-order ALM solver on the
// same velocity unknowns.  It needs the residual / gradient path only (compute_p + internal force + constraints +
// grad L: the same functions the Newton solver calls), so it is a thin loop around the Newton core's gradient
// evaluation plus the AdamW moment update; no Hessian is built or allocated.
struct tlfea_adamw_s : FirstOrder {
  tlfea_adamw_params prm{2e-4, 0.9, 0.999, 1e-8, 1e-4, 0.998, 1e-1, 1e-6, 1e14, 5, 500, 1e-3, 10, 0.0};
  double *d_m = nullptr, *d_va = nullptr;
  // 1: SyncedAdamWSolver, the cooperative-kernel sibling (SyncedAdamW.cu:96-345): same moments and step; as written
  // there the inner-converged flag is cleared once per Solve(), lam += rho dt c is applied once, and the outer loop
  // stops on ||c|| < outer_tol alone
  int coop = 0;
};

extern "C" int tlfea_adamw_create(tlfea_t10_t data, int n_constraints, tlfea_adamw_t* out) {
  tlfea_adamw_t a = fo_create<tlfea_adamw_s>("tlfea_adamw_create", data, n_constraints, out);
  if (!a) return 1;
  const size_t n = 3 * (size_t)a->core->N;
  TRY(dmalloc(&a->d_m, n));
  TRY(dmalloc(&a->d_va, n));
  HIP_TRY(hipMemset(a->d_m, 0, n * sizeof(double)));
  HIP_TRY(hipMemset(a->d_va, 0, n * sizeof(double)));
  *out = a;
  return 0;
}
extern "C" int tlfea_adamw_destroy(tlfea_adamw_t a) {
  if (!a) return 0;
  return fo_destroy(a, {a->d_m, a->d_va});
}
extern "C" int tlfea_adamw_setup(tlfea_adamw_t a) {  // Setup(): zero state (SyncedAdamWNocoop.cuh:180-198)
  const size_t n = 3 * (size_t)a->core->N;
  TRY(tlfea_newton_setup(a->core));
  HIP_TRY(hipMemset(a->d_m, 0, n * sizeof(double)));
  HIP_TRY(hipMemset(a->d_va, 0, n * sizeof(double)));
  return 0;
}
extern "C" int tlfea_adamw_set_parameters(tlfea_adamw_t a, const tlfea_adamw_params* p) {
  if (!a || !p) return fail("null argument");
  a->prm = *p;
  return fo_clear_state(a);
}
extern "C" int tlfea_adamw_set_cooperative_semantics(tlfea_adamw_t a, int on) {
  a->coop = on ? 1 : 0;
  return 0;
}
extern "C" int tlfea_adamw_set_verbose(tlfea_adamw_t a, int v) { return fo_set_verbose(a, v); }
extern "C" double* tlfea_adamw_velocity_guess_device_ptr(tlfea_adamw_t a) { return a->core->d_v; }
extern "C" int tlfea_adamw_retrieve_velocity(tlfea_adamw_t a, double* v) { return tlfea_newton_retrieve_velocity(a->core, v); }
extern "C" int tlfea_adamw_retrieve_lambda(tlfea_adamw_t a, double* lam) { return tlfea_newton_retrieve_lambda(a->core, lam); }
extern "C" int tlfea_adamw_get_stats(tlfea_adamw_t a, double* out6) { return fo_get_stats(a, out6); }

// OneStepAdamWNocoop (SyncedAdamWNocoop.cu:262-500)
extern "C" int tlfea_adamw_solve(tlfea_adamw_t a) {
  tlfea_newton_t s = a->core;
  tlfea_t10_t d = s->d;
  const tlfea_adamw_params& p = a->prm;
  if (!d->is_csr_setup) return fail("SyncedAdamWNocoop: CalcMassMatrix() must precede Solve() (the gradient uses the mass CSR)");
  if (dist_on(s)) return fail("SyncedAdamWNocoop: single-GPU path only");
  TRY(sync_constraints(s));
  const int N = s->N, n = 3 * N;
  const double dt = p.time_step;
  const int check_every = p.convergence_check_interval > 0 ? p.convergence_check_interval : 1;
  const int max_outer = s->n_constraints > 0 ? p.max_outer : 1;
  TRY(fo_begin(a, dt, p.rho));  // x_prev = x   (adamw_save_prev_pos_kernel)
  int outer_flag = 0, n_outer = 0, n_inner_total = 0, inner_flag = 0;
  double norm_g = 0.0, norm_c = 0.0;
  for (int outer = 0; outer < max_outer; outer++) {
    if (outer_flag) break;
    n_outer++;
    HIP_TRY(hipMemsetAsync(s->d_g, 0, (size_t)n * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(a->d_m, 0, (size_t)n * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(a->d_va, 0, (size_t)n * sizeof(double), s->stream));
    if (!a->coop) inner_flag = 0;
    double norm_g0 = -1.0;
    for (int inner = 0; inner < p.max_inner; inner++) {
      if (inner_flag) break;
      n_inner_total++;
      const double lr = p.lr * std::pow(p.lr_decay, inner + 1);
      const double t = (double)(inner + 2);
      const double inv1 = 1.0 / (1.0 - std::pow(p.beta1, t)), inv2 = 1.0 / (1.0 - std::pow(p.beta2, t));
      launch_adamw_update_velocity(s->stream, n, s->d_g, p.beta1, p.beta2, p.eps, p.weight_decay, lr, inv1, inv2, a->d_m,
                                   a->d_va, s->d_v);
      launch_positions_from_prev(s->stream, N, s->d_v, s->d_xp, s->d_yp, s->d_zp, dt, d->d_x, d->d_y, d->d_z);
      const bool check = (inner % check_every) == 0;
      TRY(eval_gradient(s, check ? &norm_g : nullptr));  // compute_p, f_int, constraints, grad L
      if (check) {
        double norm_v = 0.0;
        TRY(device_norm(s, s->d_v, nullptr, n, &norm_v));
        if (norm_g0 < 0.0) norm_g0 = norm_g;
        const double tol_abs = p.inner_tol * (1.0 + norm_v);
        const double tol_rel = (p.inner_rtol > 0.0 && norm_g0 > 0.0) ? p.inner_rtol * norm_g0 : 0.0;
        if (a->verbose)
          std::printf("outer iter: %d, inner iter: %d  lr: %.6e norm_g: %.17g norm_v: %.17g\n", outer, inner, lr, norm_g,
                      norm_v);
        if (norm_g <= tol_abs || (tol_rel > 0.0 && norm_g <= tol_rel)) inner_flag = 1;
      }
    }
    HIP_TRY(hipMemcpyAsync(s->d_vprev, s->d_v, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    launch_positions_from_prev(s->stream, N, s->d_v, s->d_xp, s->d_yp, s->d_zp, dt, d->d_x, d->d_y, d->d_z);
    if (s->n_constraints > 0) {
      if (d->cons_mode == 2)
        launch_lin_constraint(s->stream, d->n_constraint, d->d_joff, d->d_jcol, d->d_jval, d->d_rhs, d->d_x, d->d_y,
                              d->d_z, d->d_cons);
      else
        launch_constraint(s->stream, d->n_fixed, d->d_fixed, d->d_x, d->d_y, d->d_z, d->d_xt, d->d_yt, d->d_zt, d->d_cons);
      // adamw_dual_update_kernel adds rho*dt*c TWICE (SyncedAdamWNocoop.cu:260-264): reproduced as written
      launch_dual_update(s->stream, s->n_constraints, d->d_cons, p.rho * dt, s->d_lam);
      if (!a->coop) launch_dual_update(s->stream, s->n_constraints, d->d_cons, p.rho * dt, s->d_lam);
      TRY(device_norm(s, d->d_cons, nullptr, s->n_constraints, &norm_c));
      if (a->verbose) std::printf("norm_constraint: %.17g\n", norm_c);
      if (norm_c < p.outer_tol && (a->coop || inner_flag)) outer_flag = 1;
    }
  }
  launch_positions_from_prev(s->stream, N, s->d_v, s->d_xp, s->d_yp, s->d_zp, dt, d->d_x, d->d_y, d->d_z);
  return fo_end(a, n_outer, n_inner_total, norm_g, norm_c, inner_flag);
}


// =================================================================================================
// SyncedNesterovSolver (SyncedNesterov.cuh:26-260, SyncedNesterov.cu:95-372): accelerated gradient ALM solver on the
// velocities.  The reference runs it as one cooperative kernel with grid.sync() between phases and serial thread-0
// norms; here the same phases are ordinary launches of the engine's residual / gradient path.  Reproduced as
// written: the inner-converged flag is cleared once per Solve(), not per outer iteration (:110-113), so after the
// inner loop has converged once the later outer iterations only update the multipliers.
struct tlfea_nesterov_s : FirstOrder {
  tlfea_nesterov_params prm{1e-8, 1e14, 1e-6, 1e-6, 5, 200, 1e-3};
  double *d_vk = nullptr, *d_vkm1 = nullptr, *d_vnext = nullptr;
};
extern "C" int tlfea_nesterov_create(tlfea_t10_t data, int n_constraints, tlfea_nesterov_t* out) {
  tlfea_nesterov_t a = fo_create<tlfea_nesterov_s>("tlfea_nesterov_create", data, n_constraints, out);
  if (!a) return 1;
  const size_t n = 3 * (size_t)a->core->N;
  TRY(dmalloc(&a->d_vk, n)); TRY(dmalloc(&a->d_vkm1, n)); TRY(dmalloc(&a->d_vnext, n));
  *out = a;
  return 0;
}
extern "C" int tlfea_nesterov_destroy(tlfea_nesterov_t a) {
  if (!a) return 0;
  return fo_destroy(a, {a->d_vk, a->d_vkm1, a->d_vnext});
}
extern "C" int tlfea_nesterov_setup(tlfea_nesterov_t a) { return tlfea_newton_setup(a->core); }  // :140-156
extern "C" int tlfea_nesterov_set_parameters(tlfea_nesterov_t a, const tlfea_nesterov_params* p) {
  if (!a || !p) return fail("null argument");
  a->prm = *p;
  return fo_clear_state(a);
}
extern "C" int tlfea_nesterov_set_verbose(tlfea_nesterov_t a, int v) { return fo_set_verbose(a, v); }
extern "C" double* tlfea_nesterov_velocity_guess_device_ptr(tlfea_nesterov_t a) { return a->core->d_v; }
extern "C" int tlfea_nesterov_retrieve_velocity(tlfea_nesterov_t a, double* v) { return tlfea_newton_retrieve_velocity(a->core, v); }
extern "C" int tlfea_nesterov_retrieve_lambda(tlfea_nesterov_t a, double* lam) { return tlfea_newton_retrieve_lambda(a->core, lam); }
extern "C" int tlfea_nesterov_get_stats(tlfea_nesterov_t a, double* out6) { return fo_get_stats(a, out6); }

// OneStepNesterov (SyncedNesterov.cu:95-372)
extern "C" int tlfea_nesterov_solve(tlfea_nesterov_t a) {
  tlfea_newton_t s = a->core;
  tlfea_t10_t d = s->d;
  const tlfea_nesterov_params& p = a->prm;
  if (!d->is_csr_setup) return fail("SyncedNesterov: CalcMassMatrix() must precede Solve() (the gradient uses the mass CSR)");
  if (dist_on(s)) return fail("SyncedNesterov: single-GPU path only");
  TRY(sync_constraints(s));
  if (d->cons_mode == 2) return fail("SyncedNesterov: fixed-coefficient constraints only (as the reference, :197-200)");
  const int N = s->N, n = 3 * N;
  const double dt = p.time_step;
  const size_t nb = (size_t)n * sizeof(double);
  TRY(fo_begin(a, dt, p.rho));  // x_prev = x
  int inner_flag = 0, outer_flag = 0, n_outer = 0, n_inner_total = 0;
  double norm_g = 0.0, norm_c = 0.0;
  for (int outer = 0; outer < p.max_outer; outer++) {
    if (outer_flag) continue;
    n_outer++;
    HIP_TRY(hipMemcpyAsync(a->d_vk, s->d_v, nb, hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(a->d_vkm1, s->d_v, nb, hipMemcpyDeviceToDevice, s->stream));
    double t = 1.0, prev_norm_g = 0.0;
    for (int inner = 0; inner < p.max_inner; inner++) {
      if (inner_flag) continue;
      n_inner_total++;
      const double t_next = 0.5 * (1.0 + std::sqrt(1.0 + 4.0 * t * t)), beta = (t - 1.0) / t_next;
      launch_nesterov_lookahead(s->stream, n, beta, a->d_vk, a->d_vkm1, s->d_v);  // y -> v_guess
      launch_positions_from_prev(s->stream, N, s->d_v, s->d_xp, s->d_yp, s->d_zp, dt, d->d_x, d->d_y, d->d_z);
      TRY(eval_gradient(s, &norm_g));
      if (inner > 0 && std::fabs(norm_g - prev_norm_g) < p.inner_tol) inner_flag = 1;
      launch_nesterov_step(s->stream, n, p.alpha, s->d_v, s->d_g, a->d_vnext);
      double norm_vn = 0.0, norm_vk = 0.0;
      TRY(device_norm(s, a->d_vnext, nullptr, n, &norm_vn));
      TRY(device_norm(s, a->d_vk, nullptr, n, &norm_vk));
      if (inner > 0 && std::fabs(norm_vn - norm_vk) < p.inner_tol) inner_flag = 1;
      if (a->verbose)
        std::printf("outer iter: %d, inner iter: %d norm_g: %.17g norm_v_next: %.17g norm_v_k: %.17g\n", outer, inner,
                    norm_g, norm_vn, norm_vk);
      std::swap(a->d_vkm1, a->d_vk);   // v_km1 = v_k
      std::swap(a->d_vk, a->d_vnext);  // v_k = v_next (the old v_km1 buffer becomes scratch)
      HIP_TRY(hipMemcpyAsync(s->d_v, a->d_vk, nb, hipMemcpyDeviceToDevice, s->stream));  // v_guess = v_next
      t = t_next;
      prev_norm_g = norm_g;
    }
    HIP_TRY(hipMemcpyAsync(s->d_vprev, s->d_v, nb, hipMemcpyDeviceToDevice, s->stream));
    launch_positions_from_prev(s->stream, N, s->d_v, s->d_xp, s->d_yp, s->d_zp, dt, d->d_x, d->d_y, d->d_z);
    if (s->n_constraints > 0) {
      launch_constraint(s->stream, d->n_fixed, d->d_fixed, d->d_x, d->d_y, d->d_z, d->d_xt, d->d_yt, d->d_zt, d->d_cons);
      launch_dual_update(s->stream, s->n_constraints, d->d_cons, p.rho * dt, s->d_lam);  // lambda += rho dt c
      TRY(device_norm(s, d->d_cons, nullptr, s->n_constraints, &norm_c));
    } else {
      norm_c = 0.0;
    }
    if (a->verbose) std::printf("norm_constraint: %.17g\n", norm_c);
    if (std::fabs(norm_c) < p.outer_tol) outer_flag = 1;
  }
  launch_positions_from_prev(s->stream, N, s->d_v, s->d_xp, s->d_yp, s->d_zp, dt, d->d_x, d->d_y, d->d_z);
  return fo_end(a, n_outer, n_inner_total, norm_g, norm_c, inner_flag);
}

// =================================================================================================
// SyncedVBDSolver (SyncedVBD.cuh:13-330, SyncedVBD.cu:163-400, 764-1135, 1475-1641): vertex block descent on the same
// velocity unknowns.  One launch per colour (csrc/elem_kernels.hip vbd_color_kernel: update, position and -- implicitly,
// because it rebuilds F from the coordinates -- the reference's compute_p refresh); the convergence checks reuse the
// Newton core's gradient evaluation, the dual update its kernel.  The sweep of all colours is captured in a hipGraph,
// as the reference captures its sweep in a CUDA graph (:1233-1330).
struct tlfea_vbd_s : FirstOrder {
  tlfea_vbd_params prm{1e-4, 1e-4, 1e-4, 1e14, 5, 500, 1e-3, 1.0, 1e-12, 25, 1};
  VbdColoring col;
  std::vector<int> color_lanes;  // lanes per node of each colour's launch (16 | 32 | 64)
  int* d_color_nodes = nullptr;
  int* d_conn_rm = nullptr;   // [E][S] element-major copy of the connectivity for the sweep's gathers
  double* d_xyz = nullptr;    // [N][3] interleaved copy of the current coordinates, kept in step by the sweep
  bool coloring_ready = false, mass_ready = false, fixed_ready = false;
  int colored_group_size = 0;
  hipGraphExec_t sweep_graph = nullptr;
  // what the captured launches have baked in: h, rho, omega, hess_eps, pinned?, the data object's generation (material
  // scalars by value, the fixed-slot buffer re-allocated by UpdateNodalFixed) and the multiplier buffer
  double graph_key[7] = {0, 0, 0, 0, 0, -1, 0};
};

static void vbd_drop_graph(tlfea_vbd_t a) {
  if (a->sweep_graph) (void)hipGraphExecDestroy(a->sweep_graph);
  a->sweep_graph = nullptr;
}

extern "C" int tlfea_vbd_create(tlfea_t10_t data, int n_constraints, tlfea_vbd_t* out) {
  tlfea_vbd_t a = fo_create<tlfea_vbd_s>("tlfea_vbd_create", data, n_constraints, out);
  if (!a) return 1;
  *out = a;
  return 0;
}
extern "C" int tlfea_vbd_destroy(tlfea_vbd_t a) {
  if (!a) return 0;
  vbd_drop_graph(a);
  return fo_destroy(a, {a->d_color_nodes, a->d_conn_rm, a->d_xyz});
}
extern "C" int tlfea_vbd_setup(tlfea_vbd_t a) { return tlfea_newton_setup(a->core); }
extern "C" int tlfea_vbd_set_parameters(tlfea_vbd_t a, const tlfea_vbd_params* p) {
  if (!a || !p) return fail("null argument");
  a->prm = *p;
  if (a->prm.color_group_size <= 0) a->prm.color_group_size = 1;
  return fo_clear_state(a);
}
extern "C" int tlfea_vbd_initialize_mass_diag_blocks(tlfea_vbd_t a) {
  TRY(tlfea_t10_calc_mass_matrix(a->core->d));  // the reference recomputes the mass matrix here (:1041-1052)
  a->mass_ready = true;
  return 0;
}
extern "C" int tlfea_vbd_initialize_coloring(tlfea_vbd_t a) {
  tlfea_t10_t d = a->core->d;
  if (a->coloring_ready && a->colored_group_size == a->prm.color_group_size) return 0;
  if (!d->is_csr_setup) TRY(tlfea_vbd_initialize_mass_diag_blocks(a));  // the adjacency is the mass pattern
  if (a->verbose) std::printf("Initializing VBD coloring...\n");
  vbd_build_coloring(d->S, d->E, d->N, d->h_conn.data(), d->h_off.data(), d->h_cols.data(), a->prm.color_group_size, a->col);
  if (!a->col.valid) std::fprintf(stderr, "Warning: Invalid coloring detected!\n");
  if (a->verbose) std::printf("VBD coloring: %d colors for %d nodes\n", a->col.n_colors, d->N);
  dfree(a->d_color_nodes);
  TRY(dmalloc(&a->d_color_nodes, (size_t)d->N));
  HIP_TRY(hipMemcpy(a->d_color_nodes, a->col.color_nodes.data(), (size_t)d->N * sizeof(int), hipMemcpyHostToDevice));
  if (!a->d_conn_rm) {
    std::vector<int> rm((size_t)d->E * d->S);
    for (int e = 0; e < d->E; e++)
      for (int b = 0; b < d->S; b++) rm[(size_t)e * d->S + b] = d->h_conn[(size_t)b * d->E + e];
    TRY(dmalloc(&a->d_conn_rm, rm.size()));
    HIP_TRY(hipMemcpy(a->d_conn_rm, rm.data(), rm.size() * sizeof(int), hipMemcpyHostToDevice));
    TRY(dmalloc(&a->d_xyz, 3 * (size_t)d->N));
  }
  // lanes per node: enough for the colour's average (element, point) item count in one or two rounds
  a->color_lanes.assign((size_t)a->col.n_colors, 64);
  for (int k = 0; k < a->col.n_colors; k++) {
    double items = 0.0;
    for (int t = a->col.color_offsets[k]; t < a->col.color_offsets[k + 1]; t++) {
      const int i = a->col.color_nodes[t];
      items += (double)(d->h_n2e_off[i + 1] - d->h_n2e_off[i]) * d->Q;
    }
    const int cnt = a->col.color_offsets[k + 1] - a->col.color_offsets[k];
    const double avg = cnt ? items / cnt : 0.0;
    // narrow groups raise throughput when the colour fills the chip (config C: 12.0 -> 10.5 ms per sweep); a small
    // colour is latency-bound and finishes sooner with one round per lane (config B: 0.29 vs 0.35 ms)
    a->color_lanes[k] = cnt < 16384 ? 64 : (avg <= 20.0 ? 16 : (avg <= 40.0 ? 32 : 64));
  }
  if (const char* e = std::getenv("TLFEA_VBD_LANES")) std::fill(a->color_lanes.begin(), a->color_lanes.end(), std::atoi(e));
  a->coloring_ready = true;
  a->colored_group_size = a->prm.color_group_size;
  vbd_drop_graph(a);
  return 0;
}
extern "C" int tlfea_vbd_initialize_fixed_map(tlfea_vbd_t a) {
  tlfea_t10_t d = a->core->d;
  if (a->core->n_constraints > 0 && (!d->is_constraints_setup || d->cons_mode != 1))
    return fail("SyncedVBDSolver: pinned-node constraints (SetNodalFixed) only; the reference's fixed map has no general rows");
  a->fixed_ready = true;  // node -> slot map: built by SetNodalFixed (d_fixed_slot)
  return 0;
}
extern "C" int tlfea_vbd_coloring_sizes(tlfea_vbd_t a, int* n_colors, int* n_groups) {
  if (!a->coloring_ready) return fail("SyncedVBDSolver: InitializeColoring() has not run");
  if (n_colors) *n_colors = a->col.n_colors;
  if (n_groups) *n_groups = a->col.n_groups;
  return 0;
}
extern "C" int tlfea_vbd_retrieve_coloring(tlfea_vbd_t a, int* colors, int* color_offsets, int* color_nodes,
                                           int* group_offsets, int* group_colors) {
  if (!a->coloring_ready) return fail("SyncedVBDSolver: InitializeColoring() has not run");
  const VbdColoring& c = a->col;
  if (colors) std::copy(c.colors.begin(), c.colors.end(), colors);
  if (color_offsets) std::copy(c.color_offsets.begin(), c.color_offsets.end(), color_offsets);
  if (color_nodes) std::copy(c.color_nodes.begin(), c.color_nodes.end(), color_nodes);
  if (group_offsets) std::copy(c.group_offsets.begin(), c.group_offsets.end(), group_offsets);
  if (group_colors) std::copy(c.group_colors.begin(), c.group_colors.end(), group_colors);
  return 0;
}
extern "C" int tlfea_vbd_set_verbose(tlfea_vbd_t a, int v) { return fo_set_verbose(a, v); }
extern "C" double* tlfea_vbd_velocity_guess_device_ptr(tlfea_vbd_t a) { return a->core->d_v; }
extern "C" int tlfea_vbd_retrieve_velocity(tlfea_vbd_t a, double* v) { return tlfea_newton_retrieve_velocity(a->core, v); }
extern "C" int tlfea_vbd_retrieve_lambda(tlfea_vbd_t a, double* lam) { return tlfea_newton_retrieve_lambda(a->core, lam); }
extern "C" int tlfea_vbd_get_stats(tlfea_vbd_t a, double* out6) { return fo_get_stats(a, out6); }

// one sweep = every colour once, in group order; colours of a group share no element, so they are launched as they
// come (the reference's refresh after the group changes nothing a colour of the same group reads)
static void vbd_enqueue_sweep(tlfea_vbd_t a, hipStream_t st) {
  tlfea_newton_t s = a->core;
  tlfea_t10_t d = s->d;
  const tlfea_vbd_params& p = a->prm;
  const VbdColoring& c = a->col;
  const bool pinned = s->n_constraints > 0;
  for (int g = 0; g < c.n_groups; g++)
    for (int t = c.group_offsets[g]; t < c.group_offsets[g + 1]; t++) {
      const int k = c.group_colors[t];
      launch_vbd_color(st, a->color_lanes[k], d->view(), d->mat, d->inc(), a->d_color_nodes + c.color_offsets[k],
                       c.color_offsets[k + 1] - c.color_offsets[k], d->d_mval, d->d_fext, pinned ? d->d_fixed_slot : nullptr,
                       d->d_xt, d->d_yt, d->d_zt, s->d_lam, p.time_step, p.rho, p.omega, p.hess_eps, s->d_vprev, s->d_xp,
                       s->d_yp, s->d_zp, s->d_v, d->d_x, d->d_y, d->d_z, a->d_conn_rm, a->d_xyz, d->d_emat, d->emat_damp);
    }
}

static int vbd_sweep(tlfea_vbd_t a) {
  tlfea_newton_t s = a->core;
  const tlfea_vbd_params& p = a->prm;
  const double key[7] = {p.time_step, p.rho, p.omega, p.hess_eps, s->n_constraints > 0 ? 1.0 : 0.0, (double)s->d->gen,
                         (double)(uintptr_t)s->d_lam};
  const bool graphs = s->use_graphs && s->stream != nullptr;
  if (!graphs) {
    vbd_enqueue_sweep(a, s->stream);
    return 0;
  }
  if (a->sweep_graph && !std::equal(key, key + 7, a->graph_key)) vbd_drop_graph(a);
  if (!a->sweep_graph) {
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
    vbd_enqueue_sweep(a, s->stream);
    HIP_TRY(hipStreamEndCapture(s->stream, &graph));
    HIP_TRY(hipGraphInstantiate(&a->sweep_graph, graph, nullptr, nullptr, 0));
    HIP_TRY(hipGraphDestroy(graph));
    std::copy(key, key + 7, a->graph_key);
  }
  HIP_TRY(hipGraphLaunch(a->sweep_graph, s->stream));
  return 0;
}

// OneStepVBD (SyncedVBD.cu:1475-1641)
extern "C" int tlfea_vbd_solve(tlfea_vbd_t a) {
  tlfea_newton_t s = a->core;
  tlfea_t10_t d = s->d;
  const tlfea_vbd_params& p = a->prm;
  if (dist_on(s)) return fail("SyncedVBDSolver: single-GPU path only");
  if (d->obs.n > 0)
    return fail("SyncedVBDSolver: rigid obstacles are set, and the VBD vertex solve has no contact term; use the Newton, "
                "AdamW or Nesterov solver, or clear the obstacles");
  if (d->loads_on())
    return fail("SyncedVBDSolver: distributed loads are set, and the VBD vertex solve has no load term; use the Newton, "
                "AdamW or Nesterov solver, or clear the loads");
  TRY(sync_constraints(s));
  if (!a->mass_ready && !d->is_csr_setup) TRY(tlfea_vbd_initialize_mass_diag_blocks(a));
  if (d->is_csr_setup && d->h_off.size() == (size_t)s->N + 1) {
    // vbd_color_kernel reads every node's diagonal mass entry mval[off[i] + diagpos[i]]: a node of no element has none
    int first = -1, count = 0;
    for (int i = 0; i < s->N; i++)
      if (d->h_off[i + 1] == d->h_off[i]) {
        if (first < 0) first = i;
        count++;
      }
    if (count)
      return fail("SyncedVBDSolver: node " + std::to_string(first) + " belongs to no element (" + std::to_string(count) +
                  " such node" + (count > 1 ? "s" : "") + "): the vertex solve needs the node's diagonal mass entry, which "
                  "an empty row does not have; remove unused nodes from the mesh, or use the AdamW or Nesterov solver");
  }
  TRY(tlfea_vbd_initialize_coloring(a));
  if (!a->fixed_ready) TRY(tlfea_vbd_initialize_fixed_map(a));
  if (s->n_constraints > 0 && !d->is_constraints_setup)
    return fail("SyncedVBDSolver: n_constraints_ > 0 but constraint buffer is unavailable (did you call element constraint setup?)");
  const int N = s->N, n = 3 * N;
  const double dt = p.time_step;
  TRY(fo_begin(a, dt, p.rho));  // vbd_update_pos_prev
  int n_outer = 0, n_sweeps = 0;
  double norm_g = 0.0, norm_c = 0.0;
  for (int outer = 0; outer < p.max_outer; outer++) {
    n_outer++;
    launch_positions_from_prev(s->stream, N, s->d_v, s->d_xp, s->d_yp, s->d_zp, dt, d->d_x, d->d_y, d->d_z);
    launch_interleave_xyz(s->stream, N, d->d_x, d->d_y, d->d_z, a->d_xyz);
    double R0 = -1.0;
    if (p.convergence_check_interval > 0) {
      TRY(eval_gradient(s, &R0));
      if (a->verbose) std::printf("    [VBD check] init: ||g||=%.6e\n", R0);
    }
    for (int inner = 0; inner < p.max_inner; inner++) {
      n_sweeps++;
      TRY(vbd_sweep(a));
      if (p.convergence_check_interval > 0 && (inner % p.convergence_check_interval == 0 || inner == p.max_inner - 1)) {
        TRY(eval_gradient(s, &norm_g));
        if (a->verbose) std::printf("    VBD sweep %3d: ||g|| = %.6e\n", inner, norm_g);
        if (norm_g <= std::max(p.inner_tol, p.inner_rtol * (R0 >= 0.0 ? R0 : norm_g))) break;
      }
    }
    launch_positions_from_prev(s->stream, N, s->d_v, s->d_xp, s->d_yp, s->d_zp, dt, d->d_x, d->d_y, d->d_z);
    if (s->n_constraints > 0) {
      launch_constraint(s->stream, d->n_fixed, d->d_fixed, d->d_x, d->d_y, d->d_z, d->d_xt, d->d_yt, d->d_zt, d->d_cons);
      TRY(device_norm(s, d->d_cons, nullptr, s->n_constraints, &norm_c));
      if (a->verbose) std::printf("VBD outer %d: ||c|| = %g\n", outer, norm_c);
      if (norm_c < p.outer_tol) {
        if (a->verbose) std::printf("VBD converged at outer iteration %d\n", outer);
        break;
      }
      launch_dual_update(s->stream, s->n_constraints, d->d_cons, p.rho, s->d_lam);  // vbd_update_dual: lam += rho c
    }
  }
  HIP_TRY(hipMemcpyAsync(s->d_vprev, s->d_v, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  TRY(fo_end(a, n_outer, n_sweeps, norm_g, norm_c, 0));
  if (a->verbose) std::printf("OneStepVBD kernel time: %.3f ms\n", a->stats[5]);
  return 0;
}
