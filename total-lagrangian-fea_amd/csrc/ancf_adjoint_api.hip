// ancf_adjoint_api.hip -- C-ABI (include/tlfea_c.h) of the adjoint sensitivities of the implicit Newton step on ANCF beam
// and shell objects (DESIGN 3j').  The step itself is adjoint_step_device / adjoint_step_host of adjoint_api.hip; this unit
// holds the ANCF kind (AdjointKind, newton_handle.h): the refusals, the element kernel's launches, the stride of the
// position coefficients and the density rule.
//
// An ANCF object has one material and one density.  The stiffness slots come from ancf_sens_point_kernel at the force
// rule's points; the mass matrix is assembled on the host with a rule of its own and is linear in the density, so the
// density slot is -(M w) . u / rho0 with the density the matrix was assembled with -- one fixed-order sum, no element kernel.
#include "newton_handle.h"

static int ancf_P(tlfea_t10_t h) { return h->mat.model == kMooneyRivlin ? 3 : 2; }

// what the sensitivities need of the handle: an ANCF object, set up, with its reference gradients; then the buffers
static int ancf_sens_prepare(tlfea_t10_t h, const char* what) {
  if (h && h->kind == kT10) return fail(std::string(what) + ": ANCF handles only (not a T10 handle)");
  NEED_SETUP(h, what);
  if (!h->have_dndu) return fail(std::string(what) + ": CalcDsDuPre must be called first");
  TRY(sens_buffers(h));
  if (!h->d_sn_rho) TRY(dmalloc(&h->d_sn_rho, (size_t)h->N));
  return 0;
}
// the launches after ancf_sens_prepare: d_sn_sens [P][Epad] from the device vector w; d_sn_out [0 .. P) its sums;
// d_sn_out [P] the density slot from M w and u
static void ancf_sens_launch_points(tlfea_t10_t h, hipStream_t st, const double* d_w) {
  launch_ancf_sens_points(st, h->view(), h->mat.model, d_w, h->d_sn_sens);
}
static void ancf_sens_launch_sums(tlfea_t10_t h, hipStream_t st) {
  launch_adj_sums(st, ancf_P(h), h->E, (h->E + kAdjChunk - 1) / kAdjChunk, nullptr, nullptr, h->d_sn_sens, (size_t)h->Epad, 1, 1,
                  nullptr, h->d_sn_part, h->d_sn_out);
}
static void ancf_sens_launch_density(tlfea_t10_t h, hipStream_t st, const double* d_Mw, const double* d_u) {
  launch_ancf_rho_terms(st, h->N, d_Mw, d_u, -1.0 / h->ancf_mass_rho0, h->d_sn_rho);
  launch_adj_sums(st, 1, h->N, (h->N + kAdjChunk - 1) / kAdjChunk, nullptr, nullptr, h->d_sn_rho, 0, 1, 1, nullptr, h->d_sn_part,
                  h->d_sn_out + ancf_P(h));
}
static int ancf_density_refusal(tlfea_t10_t h, const std::string& w) {
  if (!h->ancf_mass) return fail(w + "the density slot needs the mass matrix (CalcMassMatrix) first");
  if (!(h->ancf_mass_rho0 > 0.0))
    return fail(w + "the mass matrix was assembled with density " + std::to_string(h->ancf_mass_rho0) +
                    ": the density slot divides by it (SetDensity > 0, CalcMassMatrix)");
  return 0;
}

extern "C" int tlfea_ancf_material_sensitivity_shape(tlfea_t10_t h, int* n_mat, int* slots) {
  if (h && h->kind == kT10) return fail("tlfea_ancf_material_sensitivity_shape: ANCF handles only (not a T10 handle)");
  NEED_SETUP(h, "tlfea_ancf_material_sensitivity_shape");
  if (n_mat) *n_mat = 1;
  if (slots) *slots = ancf_P(h) + 1;
  return 0;
}

extern "C" int tlfea_ancf_material_sensitivity(tlfea_t10_t h, const double* w, const double* u, double* per_element,
                                               double* per_material) {
  const char* what = "tlfea_ancf_material_sensitivity";
  TRY(ancf_sens_prepare(h, what));
  if (!w) return fail(std::string(what) + ": null w");
  if (u && per_material) TRY(ancf_density_refusal(h, std::string(what) + ": "));
  const size_t n = 3 * (size_t)h->N;
  const int P = ancf_P(h);
  if (!h->d_sn_w) TRY(dmalloc(&h->d_sn_w, n));
  if (!h->d_sn_u) TRY(dmalloc(&h->d_sn_u, n));
  HIP_TRY(hipMemcpy(h->d_sn_w, w, n * sizeof(double), hipMemcpyHostToDevice));
  ancf_sens_launch_points(h, h->stream, h->d_sn_w);
  if (per_material) {
    ancf_sens_launch_sums(h, h->stream);
    if (u) {
      double* d_Mw = nullptr;  // M w next to u
      TRY(dmalloc(&d_Mw, n));
      hipError_t e = hipMemcpy(h->d_sn_u, u, n * sizeof(double), hipMemcpyHostToDevice);
      if (e == hipSuccess) {
        launch_massmm_block(h->stream, h->N, 1, h->d_off, h->d_cols, h->d_mval, h->d_sn_w, 1, d_Mw, 1, nullptr);
        ancf_sens_launch_density(h, h->stream, d_Mw, h->d_sn_u);
        e = hipStreamSynchronize(h->stream);
      }
      (void)hipFree(d_Mw);
      HIP_TRY(e);
    } else {
      HIP_TRY(hipMemsetAsync(h->d_sn_out + P, 0, sizeof(double), h->stream));
    }
  }
  HIP_TRY(hipGetLastError());
  if (per_element) {
    if (!h->d_sn_pe) TRY(dmalloc(&h->d_sn_pe, (size_t)h->E * 4));
    launch_sens_transpose(h->stream, h->E, h->Epad, P, h->d_sn_sens, h->d_sn_pe);
    D2H(per_element, h->d_sn_pe, (size_t)h->E * P);
  }
  if (per_material) D2H(per_material, h->d_sn_out, (size_t)P + 1);
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

extern "C" int tlfea_ancf_time_sensitivity_kernels(tlfea_t10_t h, int reps, double* out_ms2) {
  const char* what = "tlfea_ancf_time_sensitivity_kernels";
  TRY(ancf_sens_prepare(h, what));
  if (!out_ms2) return fail(std::string(what) + ": null output");
  if (reps < 1) reps = 1;
  // any finite vector serves a timing: the x coordinates as the first N entries of w, zeros behind them
  const size_t n = 3 * (size_t)h->N;
  if (!h->d_sn_w) TRY(dmalloc(&h->d_sn_w, n));
  HIP_TRY(hipMemset(h->d_sn_w, 0, n * sizeof(double)));
  HIP_TRY(hipMemcpy(h->d_sn_w, h->d_x, (size_t)h->N * sizeof(double), hipMemcpyDeviceToDevice));
  TRY(time_reps(h->stream, reps, &out_ms2[0], [&](int) { ancf_sens_launch_points(h, h->stream, h->d_sn_w); return 0; }));
  TRY(time_reps(h->stream, reps, &out_ms2[1], [&](int) { ancf_sens_launch_sums(h, h->stream); return 0; }));
  return 0;
}

// ---- the ANCF kind of the adjoint step -------------------------------------------------------------------------------------
static int ancf_adjoint_refusal(tlfea_newton_t s) {
  if (!s) return fail("tlfea_newton_ancf_adjoint_step: null handle");
  tlfea_t10_t d = s->d;
  const std::string w = "tlfea_newton_ancf_adjoint_step: ";
  if (d->kind == kT10) return fail(w + "ANCF handles only (not a T10 handle)");
  TRY(adjoint_refusal_terms(s, w));
  if (!d->have_dndu) return fail(w + "needs the reference gradients (CalcDsDuPre) first");
  if (!d->is_csr_setup || !d->d_mval || !d->ancf_mass)
    return fail(w + "needs the mass matrix (BuildMassCSRPattern, CalcMassMatrix) first");
  return adjoint_refusal_state(s, w);
}
static int ancf_adjoint_prepare(tlfea_t10_t d) { return ancf_sens_prepare(d, "tlfea_newton_ancf_adjoint_step"); }
static void ancf_adjoint_materials(tlfea_t10_t d, hipStream_t st, const double* w, const double* u, const double* Mw,
                                   double* per_material, double* per_element) {
  const int P = ancf_P(d);
  ancf_sens_launch_points(d, st, w);
  if (per_material) {
    ancf_sens_launch_sums(d, st);
    ancf_sens_launch_density(d, st, Mw, u);
    (void)hipMemcpyAsync(per_material, d->d_sn_out, (size_t)(P + 1) * sizeof(double), hipMemcpyDeviceToDevice, st);
  }
  if (per_element) launch_sens_transpose(st, d->E, d->Epad, P, d->d_sn_sens, per_element);
}
static size_t ancf_pm_doubles(tlfea_t10_t d) { return (size_t)ancf_P(d) + 1; }
static size_t ancf_pe_doubles(tlfea_t10_t d) { return (size_t)d->E * ancf_P(d); }
static const AdjointKind kAncfAdjoint{"tlfea_newton_ancf_adjoint_step", 4, ancf_adjoint_refusal, ancf_adjoint_prepare,
                                     ancf_adjoint_materials, ancf_pm_doubles, ancf_pe_doubles};

extern "C" int tlfea_newton_ancf_adjoint_ready(tlfea_newton_t s) { return ancf_adjoint_refusal(s); }

// the density slot divides by the density of the assembled mass matrix: refused only where per_material is wanted
static int ancf_adjoint_wanted(tlfea_newton_t s, const tlfea_adjoint_out* out) {
  TRY(ancf_adjoint_refusal(s));
  if (out && out->per_material) TRY(ancf_density_refusal(s->d, "tlfea_newton_ancf_adjoint_step: "));
  return 0;
}

extern "C" int tlfea_newton_ancf_adjoint_step_device(tlfea_newton_t s, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out,
                                                     int* info, double* rel_res) {
  TRY(ancf_adjoint_wanted(s, out));
  return adjoint_step_device(s, kAncfAdjoint, in, out, nullptr, info, rel_res);
}

extern "C" int tlfea_newton_ancf_adjoint_step(tlfea_newton_t s, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out, int* info,
                                              double* rel_res) {
  TRY(ancf_adjoint_wanted(s, out));
  return adjoint_step_host(s, kAncfAdjoint, in, out, nullptr, info, rel_res);
}
