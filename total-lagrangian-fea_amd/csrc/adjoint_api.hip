// adjoint_api.hip -- adjoint of the implicit Newton step: material and shape sensitivities of a T10 object,
// the step shared by every element kind and the T10 kind's entry points (ancf_adjoint_api.hip holds the ANCF kind).  The
// reference (SyncedNewton.cu) has no adjoint.
#include "newton_handle.h"

using namespace tlfea;

// =================================================================================================
// Adjoint sensitivities of the implicit step (adjoint_kernels.hip)
static int sens_slots(tlfea_t10_t h) { return (h->mat.model == kMooneyRivlin ? 3 : 2) + 1; }
static int sens_n_mat(tlfea_t10_t h) { return h->d_emat ? h->n_mat : 1; }
// what both sensitivities need of the handle: a T10 mesh, set up, with its reference-geometry tables
static int sens_need_t10(tlfea_t10_t h, const char* what) {
  if (h && h->kind != kT10) return fail(std::string(what) + ": T10 handles only (not an ANCF handle)");
  NEED_SETUP(h, what);
  if (!h->have_dndu) return fail(std::string(what) + ": CalcDnDuPre must be called first");
  return 0;
}
// the vectors of the two timing entry points -- any finite ones serve a timing: the positions as w, zeros as u
static int sens_timing_vectors(tlfea_t10_t h) {
  const size_t n = 3 * (size_t)h->N;
  if (!h->d_sn_w) TRY(dmalloc(&h->d_sn_w, n));
  if (!h->d_sn_u) TRY(dmalloc(&h->d_sn_u, n));
  HIP_TRY(hipMemset(h->d_sn_w, 0, n * sizeof(double)));
  HIP_TRY(hipMemcpy(h->d_sn_w, h->d_x, (size_t)h->N * sizeof(double), hipMemcpyDeviceToDevice));
  HIP_TRY(hipMemset(h->d_sn_u, 0, n * sizeof(double)));
  return 0;
}
// buffers and, under a material table, the ascending element list of every material with its chunks of kAdjChunk (any
// element kind; newton_handle.h)
int tlfea::sens_buffers(tlfea_t10_t h) {
  if (!h->d_sn_sens) TRY(dmalloc(&h->d_sn_sens, (size_t)4 * h->Epad));
  const int n_mat = sens_n_mat(h);
  if (n_mat > h->sn_out_cap) {
    if (h->d_sn_out) (void)hipFree(h->d_sn_out);
    TRY(dmalloc(&h->d_sn_out, (size_t)n_mat * 4));
    h->sn_out_cap = n_mat;
  }
  int nb = (h->E + kAdjChunk - 1) / kAdjChunk;
  if (h->d_emat && h->sn_gen != h->gen) {
    std::vector<int> cnt(n_mat + 1, 0), idx(h->E), boff(n_mat + 1, 0);
    for (int e = 0; e < h->E; e++) cnt[h->h_eid[e] + 1]++;
    for (int k = 0; k < n_mat; k++) cnt[k + 1] += cnt[k];
    std::vector<int> at(cnt.begin(), cnt.end() - 1);
    for (int e = 0; e < h->E; e++) idx[at[h->h_eid[e]]++] = e;  // ascending inside every material
    std::vector<int2> blk;
    for (int k = 0; k < n_mat; k++) {
      boff[k] = (int)blk.size();
      for (int a = cnt[k]; a < cnt[k + 1]; a += kAdjChunk) blk.push_back(make_int2(a, std::min(cnt[k + 1], a + kAdjChunk)));
    }
    boff[n_mat] = (int)blk.size();
    HIP_TRY(hipDeviceSynchronize());
    dfree(h->d_sn_idx);
    dfree(h->d_sn_boff);
    dfree(h->d_sn_blk);
    TRY(dmalloc(&h->d_sn_idx, idx.size()));
    TRY(dmalloc(&h->d_sn_boff, boff.size()));
    TRY(dmalloc(&h->d_sn_blk, blk.size()));
    HIP_TRY(hipMemcpy(h->d_sn_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_sn_boff, boff.data(), boff.size() * sizeof(int), hipMemcpyHostToDevice));
    if (!blk.empty()) HIP_TRY(hipMemcpy(h->d_sn_blk, blk.data(), blk.size() * sizeof(int2), hipMemcpyHostToDevice));
    h->sn_nb = (int)blk.size();
    h->sn_gen = h->gen;
  }
  if (h->d_emat) nb = h->sn_nb;
  const int cap = std::max(nb, (h->N + kAdjChunk - 1) / kAdjChunk);  // the node sums of a_bar share the buffer
  if (cap > h->sn_part_cap) {
    if (h->d_sn_part) (void)hipFree(h->d_sn_part);
    TRY(dmalloc(&h->d_sn_part, (size_t)cap * 4));
    h->sn_part_cap = cap;
  }
  return 0;
}
static int sens_prepare(tlfea_t10_t h, const char* what) {
  TRY(sens_need_t10(h, what));
  return sens_buffers(h);
}
// the two launches after sens_prepare: d_sn_sens from device vectors w, u, then d_sn_out [n_mat][slots]
static void sens_launch_points(tlfea_t10_t h, hipStream_t st, const double* d_w, const double* d_u) {
  SensShape sh;
  shape_at_rule_points(h, sh.Nq);
  launch_sens_points(st, h->view(), h->mat.model, sh, d_w, d_u, h->d_sn_sens);
}
static void sens_launch_sums(tlfea_t10_t h, hipStream_t st) {
  if (h->d_emat)
    launch_adj_sums(st, sens_slots(h), h->E, h->sn_nb, h->d_sn_blk, h->d_sn_idx, h->d_sn_sens, (size_t)h->Epad, 1, h->n_mat,
                    h->d_sn_boff, h->d_sn_part, h->d_sn_out);
  else
    launch_adj_sums(st, sens_slots(h), h->E, (h->E + kAdjChunk - 1) / kAdjChunk, nullptr, nullptr, h->d_sn_sens,
                    (size_t)h->Epad, 1, 1, nullptr, h->d_sn_part, h->d_sn_out);
}

extern "C" int tlfea_t10_material_sensitivity_shape(tlfea_t10_t h, int* n_mat, int* slots) {
  if (h && h->kind != kT10) return fail("tlfea_t10_material_sensitivity_shape: T10 handles only (not an ANCF handle)");
  NEED_SETUP(h, "tlfea_t10_material_sensitivity_shape");
  if (n_mat) *n_mat = sens_n_mat(h);
  if (slots) *slots = sens_slots(h);
  return 0;
}

extern "C" int tlfea_t10_material_sensitivity(tlfea_t10_t h, const double* w, const double* u, double* per_element,
                                              double* per_material) {
  TRY(sens_prepare(h, "tlfea_t10_material_sensitivity"));
  if (!w) return fail("tlfea_t10_material_sensitivity: null w");
  const size_t n = 3 * (size_t)h->N;
  if (!h->d_sn_w) TRY(dmalloc(&h->d_sn_w, n));
  if (u && !h->d_sn_u) TRY(dmalloc(&h->d_sn_u, n));
  HIP_TRY(hipMemcpy(h->d_sn_w, w, n * sizeof(double), hipMemcpyHostToDevice));
  if (u) HIP_TRY(hipMemcpy(h->d_sn_u, u, n * sizeof(double), hipMemcpyHostToDevice));
  const int slots = sens_slots(h);
  sens_launch_points(h, h->stream, h->d_sn_w, u ? h->d_sn_u : nullptr);
  sens_launch_sums(h, h->stream);
  HIP_TRY(hipGetLastError());
  if (per_element) {
    if (!h->d_sn_pe) TRY(dmalloc(&h->d_sn_pe, (size_t)h->E * 4));
    launch_sens_transpose(h->stream, h->E, h->Epad, slots, h->d_sn_sens, h->d_sn_pe);
    D2H(per_element, h->d_sn_pe, (size_t)h->E * slots);
  }
  if (per_material) D2H(per_material, h->d_sn_out, (size_t)sens_n_mat(h) * slots);
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

extern "C" int tlfea_t10_time_sensitivity_kernels(tlfea_t10_t h, int reps, double* out_ms2) {
  TRY(sens_prepare(h, "tlfea_t10_time_sensitivity_kernels"));
  if (!out_ms2) return fail("tlfea_t10_time_sensitivity_kernels: null output");
  if (reps < 1) reps = 1;
  TRY(sens_timing_vectors(h));
  TRY(time_reps(h->stream, reps, &out_ms2[0], [&](int) { sens_launch_points(h, h->stream, h->d_sn_w, h->d_sn_u); return 0; }));
  TRY(time_reps(h->stream, reps, &out_ms2[1], [&](int) { sens_launch_sums(h, h->stream); return 0; }));
  return 0;
}

// ---- shape sensitivities (shape_kernels.hip) -----------------------------------------------------------------
static int shape_prepare(tlfea_t10_t h, const char* what) {
  TRY(sens_need_t10(h, what));
  if (!h->is_csr_setup) TRY(tlfea_t10_build_mass_csr_pattern(h));  // the node -> element incidence of the gather
  if (!h->d_sh_rows) TRY(dmalloc(&h->d_sh_rows, (size_t)3 * kNN * h->Epad));
  return 0;
}
// the two launches after shape_prepare: device vectors w, u [3N] (u null: no mass term) -> d_xbar [N][3].  The density
// of the mass term is the one the mass matrix was assembled with.
static void shape_launch_points(tlfea_t10_t h, hipStream_t st, const double* d_w, const double* d_u) {
  Material m = h->mat;
  m.rho0 = h->mass_rho0 >= 0.0 ? h->mass_rho0 : 0.0;
  launch_shape_points(st, h->view(), m, h->d_emat, h->h_q, d_w, d_u, h->d_sh_rows);
}
static void shape_launch_gather(tlfea_t10_t h, hipStream_t st, double* d_xbar) {
  launch_shape_gather(st, h->N, h->Epad, h->inc(), h->d_sh_rows, d_xbar);
}

extern "C" int tlfea_t10_shape_sensitivity(tlfea_t10_t h, const double* w, const double* u, double* X_bar) {
  TRY(shape_prepare(h, "tlfea_t10_shape_sensitivity"));
  if (!w || !X_bar) return fail("tlfea_t10_shape_sensitivity: null w or X_bar");
  if (u && h->mass_rho0 < 0.0) return fail("tlfea_t10_shape_sensitivity: u given but no mass matrix is assembled (CalcMassMatrix)");
  const size_t n = 3 * (size_t)h->N;
  if (!h->d_sn_w) TRY(dmalloc(&h->d_sn_w, n));
  if (u && !h->d_sn_u) TRY(dmalloc(&h->d_sn_u, n));
  if (!h->d_sh_out) TRY(dmalloc(&h->d_sh_out, n));
  HIP_TRY(hipMemcpy(h->d_sn_w, w, n * sizeof(double), hipMemcpyHostToDevice));
  if (u) HIP_TRY(hipMemcpy(h->d_sn_u, u, n * sizeof(double), hipMemcpyHostToDevice));
  shape_launch_points(h, h->stream, h->d_sn_w, u ? h->d_sn_u : nullptr);
  shape_launch_gather(h, h->stream, h->d_sh_out);
  HIP_TRY(hipGetLastError());
  D2H(X_bar, h->d_sh_out, n);
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

extern "C" int tlfea_t10_time_shape_kernels(tlfea_t10_t h, int reps, double* out_ms2) {
  TRY(shape_prepare(h, "tlfea_t10_time_shape_kernels"));
  if (!out_ms2) return fail("tlfea_t10_time_shape_kernels: null output");
  if (reps < 1) reps = 1;
  TRY(sens_timing_vectors(h));
  if (!h->d_sh_out) TRY(dmalloc(&h->d_sh_out, 3 * (size_t)h->N));
  TRY(time_reps(h->stream, reps, &out_ms2[0], [&](int) { shape_launch_points(h, h->stream, h->d_sn_w, h->d_sn_u); return 0; }));
  TRY(time_reps(h->stream, reps, &out_ms2[1], [&](int) { shape_launch_gather(h, h->stream, h->d_sh_out); return 0; }));
  return 0;
}

// why the adjoint step cannot run on the solver's state now (0: it can)
static int adjoint_refusal(tlfea_newton_t s) {
  if (!s) return fail("tlfea_newton_adjoint_step: null handle");
  tlfea_t10_t d = s->d;
  const std::string w = "tlfea_newton_adjoint_step: ";
  if (d->kind != kT10) return fail(w + "T10 handles only (not an ANCF handle)");
  TRY(adjoint_refusal_terms(s, w));
  if (!d->have_dndu || !d->is_csr_setup || !d->d_mval || d->mass_rho0 < 0.0)
    return fail(w + "needs the mass matrix (CalcDnDuPre, CalcMassMatrix) first");
  return adjoint_refusal_state(s, w);
}
// the terms of the step the adjoint does not carry, on any element kind (w: the entry point's name and ": ")
int tlfea::adjoint_refusal_terms(tlfea_newton_t s, const std::string& w) {
  tlfea_t10_t d = s->d;
  if (d->mat.eta != 0.0 || d->mat.lamd != 0.0 || d->emat_damp)
    return fail(w + "damping is set (eta / lambda_damp != 0, uniform or in the material table): the viscous stress depends "
                    "on v and x separately, which the adjoint of the undamped step does not carry");
  for (int k = 0; k < d->obs.n; k++)
    if (d->obs.o[k].mu > 0.0)
      return fail(w + "obstacle " + std::to_string(k) + " has friction: its force depends on the start-of-step positions "
                      "and its step is line-searched; frictionless obstacles only");
  if (d->ld_n_press > 0)
    return fail(w + "a follower pressure is set: its load stiffness is not in H, so H is not the Jacobian of the residual");
  if (dist_on(s)) return fail(w + "not available on a partitioned mesh (set_interface / set_halo is active)");
  return 0;
}
// what the last Solve() left
int tlfea::adjoint_refusal_state(tlfea_newton_t s, const std::string& w) {
  switch (s->adj_state) {
    case 1: break;
    case 0: return fail(w + "no Solve() has run: the state must be that of a step just solved");
    case 2: return fail(w + "the last Solve() ran more than one outer iteration: one differentiated step is one outer "
                            "iteration (max_outer = 1)");
    case 3: return fail(w + "the last Solve() failed");
    default: return fail(w + "the last Solve() left its Newton loop without meeting inner_atol / inner_rtol: H is the "
                             "Jacobian of the residual at a converged step only");
  }
  return 0;
}
extern "C" int tlfea_newton_adjoint_ready(tlfea_newton_t s) { return adjoint_refusal(s); }
// what X_bar adds to the refusals: loads whose nodal weights are reference areas, which the shape kernel does not carry
static int adjoint_shape_refusal(tlfea_newton_t s) {
  tlfea_t10_t d = s->d;
  const std::string w = "tlfea_newton_adjoint_step_shape: ";
  if (d->obs.n > 0)
    return fail(w + "a rigid or field obstacle is set: its nodal weights are reference areas, whose dependence on the "
                    "reference geometry X_bar does not carry");
  if (d->ld_n_trac > 0)
    return fail(w + "a face traction is set: its nodal loads are reference areas, whose dependence on the reference "
                    "geometry X_bar does not carry");
  return 0;
}

// the T10 kind of the adjoint step (AdjointKind, newton_handle.h): the material slots come from sens_point_kernel, the
// density slot among them
static int t10_adjoint_prepare(tlfea_t10_t d) { return sens_prepare(d, "tlfea_newton_adjoint_step"); }
static void t10_adjoint_materials(tlfea_t10_t d, hipStream_t st, const double* w, const double* u, const double*,
                                  double* per_material, double* per_element) {
  const int slots = sens_slots(d);
  sens_launch_points(d, st, w, u);
  if (per_material) {
    sens_launch_sums(d, st);
    (void)hipMemcpyAsync(per_material, d->d_sn_out, (size_t)sens_n_mat(d) * slots * sizeof(double), hipMemcpyDeviceToDevice, st);
  }
  if (per_element) launch_sens_transpose(st, d->E, d->Epad, slots, d->d_sn_sens, per_element);
}
static size_t t10_pm_doubles(tlfea_t10_t d) { return (size_t)sens_n_mat(d) * sens_slots(d); }
static size_t t10_pe_doubles(tlfea_t10_t d) { return (size_t)d->E * sens_slots(d); }
static const AdjointKind kT10Adjoint{"tlfea_newton_adjoint_step", 1, adjoint_refusal, t10_adjoint_prepare, t10_adjoint_materials,
                                    t10_pm_doubles, t10_pe_doubles};

// The adjoint step on device pointers, for the element kind K (X_bar: T10 only).
int tlfea::adjoint_step_device(tlfea_newton_t s, const AdjointKind& K, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out,
                               double* X_bar, int* info, double* rel_res) {
  TRY(K.refusal(s));
  const std::string what = K.what;
  if (!in || !out) return fail(what + ": null argument");
  tlfea_t10_t d = s->d;
  if (X_bar) {
    TRY(adjoint_shape_refusal(s));
    TRY(shape_prepare(d, "tlfea_newton_adjoint_step_shape"));
  }
  TRY(K.prepare(d));
  TRY(tlfea_newton_analyze_hessian_sparsity(s));
  TRY(sync_constraints(s));
  const int n = 3 * s->N, nc = s->n_constraints;
  const double h = s->prm.time_step, rho = s->prm.rho;
  const double* vprev = in->v_prev ? in->v_prev : (s->d_step0 ? s->d_step0 + n : nullptr);
  if (!vprev) return fail(what + ": no v_prev given and no Solve() has kept one");
  AdjCons J{0, d->d_fixed, d->d_fixed_slot, d->d_joff, d->d_jcol, d->d_jtoff, d->d_jtcol, d->d_jval, d->d_jtval};
  J.mode = pinned_on(s) ? 1 : (lincons_on(s) ? 2 : 0);
  const double zero3[3] = {0.0, 0.0, 0.0};
  ModalWork wk;
  double *xt, *vt, *u, *Mw;
  TRY(wk.alloc(&xt, (size_t)n));
  TRY(wk.alloc(&vt, (size_t)n));
  TRY(wk.alloc(&u, (size_t)n));
  TRY(wk.alloc(&Mw, (size_t)n));
  // what the call must leave as it found it: the warm-start state of the linear solver (tlfea_newton_modal_solve)
  LamKeep keep;
  TRY(keep.save(s, wk, /*solve_state=*/true));  // cold estimates: the result depends on no earlier solve
  launch_adj_rhs(s->stream, n, J, in->x_bar, in->v_bar, J.mode ? in->lam_bar : nullptr, s->d_v, vprev,
                 d->ld_have_a ? d->ld_a : zero3, K.stride, h, rho, xt, vt, u);
  int it = 0;
  double rel = 0.0;
  int rc = assemble(s, /*fq_fresh=*/false);
  // the solve runs on the Newton iteration's own right-hand side and solution vectors (scratch between Solve() calls), so
  // the captured CG graphs stay those of the forward step
  if (!rc && hipMemcpyAsync(s->d_b, vt, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream) != hipSuccess)
    rc = fail(what + ": device copy failed");
  if (!rc) rc = pcg(s, s->d_b, s->d_dv, &it, &rel);
  const std::string why = rc ? api_error() : std::string();
  if (rc) {
    (void)hipStreamSynchronize(s->stream);
    keep.restore();
    api_error() = why;
    return rc;
  }
  const double* w = s->d_dv;
  launch_massmm_block(s->stream, s->N, 1, d->d_off, d->d_cols, d->d_mval, w, 1, Mw, 1, nullptr);
  launch_adj_out(s->stream, n, nc, J, w, Mw, xt, vt, J.mode ? in->lam_bar : nullptr, h, rho, out->f_ext_bar,
                 out->v_prev_bar, out->x_prev_bar, out->lam_in_bar, out->t_bar);
  if (J.mode == 0 && nc > 0) {  // constraint terms off: the multipliers pass through
    for (double* p : {out->lam_in_bar, out->t_bar})
      if (p) (void)hipMemsetAsync(p, 0, (size_t)nc * sizeof(double), s->stream);
  }
  if (out->a_bar) {  // over the position coefficients: every K.stride-th coefficient vector
    const int n_pos = s->N / K.stride;
    launch_adj_sums(s->stream, 3, n_pos, (n_pos + kAdjChunk - 1) / kAdjChunk, nullptr, nullptr, Mw, 1, 3 * K.stride, 1, nullptr,
                    d->d_sn_part, out->a_bar);
  }
  if (out->per_material || out->per_element) K.materials(d, s->stream, w, u, Mw, out->per_material, out->per_element);
  if (X_bar) {
    shape_launch_points(d, s->stream, w, u);
    shape_launch_gather(d, s->stream, X_bar);
  }
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(s->stream);
  keep.restore();
  HIP_TRY(e1);
  HIP_TRY(e2);
  if (info) info[0] = it;
  if (rel_res) *rel_res = rel;
  return 0;
}

extern "C" int tlfea_newton_adjoint_step_shape_device(tlfea_newton_t s, const tlfea_adjoint_in* in,
                                                      const tlfea_adjoint_out* out, double* X_bar, int* info, double* rel_res) {
  return adjoint_step_device(s, kT10Adjoint, in, out, X_bar, info, rel_res);
}

extern "C" int tlfea_newton_adjoint_step_device(tlfea_newton_t s, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out,
                                                int* info, double* rel_res) {
  return adjoint_step_device(s, kT10Adjoint, in, out, nullptr, info, rel_res);
}

// The same on host arrays: device copies of what is given and wanted around adjoint_step_device.
int tlfea::adjoint_step_host(tlfea_newton_t s, const AdjointKind& K, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out,
                             double* X_bar, int* info, double* rel_res) {
  TRY(K.refusal(s));
  if (!in || !out) return fail(std::string(K.what) + ": null argument");
  tlfea_t10_t d = s->d;
  if (X_bar) TRY(adjoint_shape_refusal(s));
  const size_t n = 3 * (size_t)s->N, nc = (size_t)s->n_constraints;
  const size_t n_pm = K.pm_doubles(d), n_pe = K.pe_doubles(d);
  ModalWork wk;
  tlfea_adjoint_in din{nullptr, nullptr, nullptr, nullptr};
  tlfea_adjoint_out dout{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  auto up = [&](const double* src, size_t cnt, const double** dst) -> int {
    if (!src || cnt == 0) return 0;
    double* p;
    TRY(wk.alloc(&p, cnt));
    HIP_TRY(hipMemcpy(p, src, cnt * sizeof(double), hipMemcpyHostToDevice));
    *dst = p;
    return 0;
  };
  TRY(up(in->x_bar, n, &din.x_bar));
  TRY(up(in->v_bar, n, &din.v_bar));
  TRY(up(in->lam_bar, nc, &din.lam_bar));
  TRY(up(in->v_prev, n, &din.v_prev));
  struct Ret { double* host; double** dev; size_t cnt; };
  double* d_Xbar = nullptr;
  const Ret rets[] = {{out->f_ext_bar, &dout.f_ext_bar, n}, {out->v_prev_bar, &dout.v_prev_bar, n},
                      {out->x_prev_bar, &dout.x_prev_bar, n}, {out->lam_in_bar, &dout.lam_in_bar, nc},
                      {out->t_bar, &dout.t_bar, nc}, {out->a_bar, &dout.a_bar, 3},
                      {out->per_material, &dout.per_material, n_pm}, {out->per_element, &dout.per_element, n_pe},
                      {X_bar, &d_Xbar, n}};
  for (const Ret& r : rets)
    if (r.host && r.cnt > 0) TRY(wk.alloc(r.dev, r.cnt));
  TRY(adjoint_step_device(s, K, &din, &dout, d_Xbar, info, rel_res));
  for (const Ret& r : rets)
    if (r.host && r.cnt > 0) HIP_TRY(hipMemcpy(r.host, *r.dev, r.cnt * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int tlfea_newton_adjoint_step_shape(tlfea_newton_t s, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out,
                                               double* X_bar, int* info, double* rel_res) {
  return adjoint_step_host(s, kT10Adjoint, in, out, X_bar, info, rel_res);
}

extern "C" int tlfea_newton_adjoint_step(tlfea_newton_t s, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out,
                                         int* info, double* rel_res) {
  return adjoint_step_host(s, kT10Adjoint, in, out, nullptr, info, rel_res);
}
