// stress_recovery_api.hip -- C-ABI (include/tlfea_c.h) of the recovered nodal stress, the principal stresses and the ZZ
// error indicator of T10 objects (DESIGN 3f'').
#include "data_handle.h"

using namespace tlfea;

// T [10][5]: the unweighted least-squares fit, linear in the reference coordinates, of the values at the rule's points,
// evaluated at the vertices (the rows of pinv(B), B [5][4] the points' barycentric coordinates) and at the mid-edge nodes
// (the mean of the two vertex rows); Nq: the shape functions at the points.  From the rule the object was set up with.
static int recovery_table(tlfea_t10_t h, RecoveryTable& tb) {
  const int edges[6][2] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {1, 3}, {2, 3}};  // local order of the mid-edge nodes
  double B[kNQ][4], M[4][4 + kNQ];  // M = [B^T B | B^T], reduced to [I | pinv(B)]
  for (int q = 0; q < kNQ; q++) {
    B[q][0] = 1.0 - h->h_q[0][q] - h->h_q[1][q] - h->h_q[2][q];
    for (int d = 0; d < 3; d++) B[q][d + 1] = h->h_q[d][q];
    for (int k = 0; k < 4; k++) tb.Nq[q][k] = B[q][k] * (2.0 * B[q][k] - 1.0);
    for (int k = 0; k < 6; k++) tb.Nq[q][k + 4] = 4.0 * B[q][edges[k][0]] * B[q][edges[k][1]];
    tb.qw[q] = h->h_qw[q];
  }
  for (int i = 0; i < 4; i++) {
    for (int j = 0; j < 4; j++) {
      M[i][j] = 0.0;
      for (int q = 0; q < kNQ; q++) M[i][j] += B[q][i] * B[q][j];
    }
    for (int q = 0; q < kNQ; q++) M[i][4 + q] = B[q][i];
  }
  for (int c = 0; c < 4; c++) {  // Gauss-Jordan with partial pivoting
    int p = c;
    for (int r = c + 1; r < 4; r++)
      if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
    if (!(std::fabs(M[p][c]) > 1e-14))
      return fail("tlfea_t10_recover_stress: the quadrature points do not span the element (no linear fit exists)");
    for (int j = 0; j < 4 + kNQ; j++) std::swap(M[c][j], M[p][j]);
    const double ip = 1.0 / M[c][c];
    for (int j = 0; j < 4 + kNQ; j++) M[c][j] *= ip;
    for (int r = 0; r < 4; r++) {
      if (r == c) continue;
      const double f = M[r][c];
      for (int j = 0; j < 4 + kNQ; j++) M[r][j] -= f * M[c][j];
    }
  }
  for (int q = 0; q < kNQ; q++) {
    for (int b = 0; b < 4; b++) tb.T[b][q] = M[b][4 + q];
    for (int k = 0; k < 6; k++) tb.T[4 + k][q] = 0.5 * (M[edges[k][0]][4 + q] + M[edges[k][1]][4 + q]);
  }
  return 0;
}

static int recovery_prepare(tlfea_t10_t h, const std::string& what, bool own_points, int want_principal,
                            int want_directions) {
  if (h && h->kind != kT10) return fail(what + ": T10 handles only (not an ANCF handle)");
  NEED_SETUP(h, what);
  if (own_points) {
    if (!h->st_valid) return fail(what + ": tlfea_t10_calc_stress has not been called");
    if (!h->st_pts_valid)
      return fail(what + ": the last tlfea_t10_calc_stress did not ask for point stresses (want_points = 0)");
  } else if (!h->have_dndu) {
    return fail(what + ": CalcDnDuPre must be called first");
  }
  if (!h->is_csr_setup) TRY(tlfea_t10_build_mass_csr_pattern(h));  // the node -> element incidence of the nodal gather
  if (!h->d_rc_rec) {
    TRY(dmalloc(&h->d_rc_rec, (size_t)h->E * kRecoveryRec));
    TRY(dmalloc(&h->d_rc_nodal, (size_t)h->N * 7));
    TRY(dmalloc(&h->d_rc_err, (size_t)3 * h->Epad));
    TRY(dmalloc(&h->d_rc_part, (size_t)3 * ((h->E + kAdjChunk - 1) / kAdjChunk)));
    TRY(dmalloc(&h->d_rc_tot, (size_t)3));
  }
  if (want_principal && !h->d_rc_pn) {
    TRY(dmalloc(&h->d_rc_pn, (size_t)h->N * 4));
    TRY(dmalloc(&h->d_rc_pe, (size_t)h->E * 4));
  }
  if (want_directions && !h->d_rc_dn) {
    TRY(dmalloc(&h->d_rc_dn, (size_t)h->N * 9));
    TRY(dmalloc(&h->d_rc_de, (size_t)h->E * 9));
  }
  return 0;
}
// stage 0 element records, 1 nodal gather, 2 principal stresses, 3 error indicator, 4 its totals
static void recovery_launch(tlfea_t10_t h, const RecoveryTable& tb, const double* d_pts, int want_principal,
                            int want_directions, int stage) {
  hipStream_t s = h->stream;
  if (stage == 0) launch_recovery_elem(s, h->E, h->d_detJ, tb, d_pts, h->d_rc_rec);
  else if (stage == 1) launch_recovery_nodal(s, h->N, h->inc(), h->d_rc_rec, h->d_rc_nodal);
  else if (stage == 2) {
    if (!want_principal) return;
    launch_principal(s, h->N, h->d_rc_nodal, 7, 0, h->d_rc_pn, want_directions ? h->d_rc_dn : nullptr);
    launch_principal(s, h->E, h->d_rc_rec, kRecoveryRec, 26, h->d_rc_pe, want_directions ? h->d_rc_de : nullptr);
  } else if (stage == 3) launch_zz_error(s, h->view(), h->mat, h->d_emat, tb, d_pts, h->d_rc_nodal, h->d_rc_err);
  else
    launch_adj_sums(s, 3, h->E, (h->E + kAdjChunk - 1) / kAdjChunk, nullptr, nullptr, h->d_rc_err, (size_t)h->Epad, 1, 1,
                    nullptr, h->d_rc_part, h->d_rc_tot);
}
static int recovery_done(tlfea_t10_t h, int want_principal, int want_directions) {
  double t[3];
  HIP_TRY(hipMemcpy(t, h->d_rc_tot, sizeof(t), hipMemcpyDeviceToHost));
  h->rc_tot[0] = t[0];
  h->rc_tot[1] = t[1];
  h->rc_tot[2] = (t[0] + t[1]) > 0.0 ? std::sqrt(t[0] / (t[1] + t[0])) : 0.0;
  h->rc_tot[3] = t[2];
  h->rc_valid = true;
  h->rc_principal = want_principal != 0;
  h->rc_directions = want_directions != 0;
  return 0;
}
static int recover(tlfea_t10_t h, const std::string& what, const double* points, bool own_points, int want_principal,
                   int want_directions) {
  want_principal |= want_directions;
  TRY(recovery_prepare(h, what, own_points, want_principal, want_directions));
  const double* d_pts = h->d_st_pts;
  if (!own_points) {
    if (!points) return fail(what + ": null points");
    if (!h->d_rc_pts) TRY(dmalloc(&h->d_rc_pts, (size_t)h->E * kNQ * 6));
    HIP_TRY(hipMemcpy(h->d_rc_pts, points, (size_t)h->E * kNQ * 6 * sizeof(double), hipMemcpyHostToDevice));
    d_pts = h->d_rc_pts;
  }
  RecoveryTable tb;
  TRY(recovery_table(h, tb));
  h->rc_valid = false;
  for (int stage = 0; stage < 5; stage++) recovery_launch(h, tb, d_pts, want_principal, want_directions, stage);
  HIP_TRY(hipGetLastError());
  return recovery_done(h, want_principal, want_directions);
}
static int need_recovery(tlfea_t10_t h, const std::string& what) {
  if (h && h->kind != kT10) return fail(what + ": T10 handles only (not an ANCF handle)");
  if (!h || !h->rc_valid) return fail(what + ": tlfea_t10_recover_stress has not been called");
  return 0;
}

extern "C" int tlfea_t10_recover_stress(tlfea_t10_t h, int want_principal, int want_directions) {
  return recover(h, "tlfea_t10_recover_stress", nullptr, true, want_principal, want_directions);
}
extern "C" int tlfea_t10_recover_stress_from_points(tlfea_t10_t h, const double* points, int want_principal,
                                                    int want_directions) {
  return recover(h, "tlfea_t10_recover_stress_from_points", points, false, want_principal, want_directions);
}
extern "C" int tlfea_t10_retrieve_recovered_stress(tlfea_t10_t h, double* sigma, double* von_mises) {
  TRY(need_recovery(h, "tlfea_t10_retrieve_recovered_stress"));
  std::vector<double> rec((size_t)h->N * 7);
  D2H(rec.data(), h->d_rc_nodal, rec.size());
  for (int i = 0; i < h->N; i++) {
    if (sigma) std::copy_n(&rec[(size_t)i * 7], 6, sigma + (size_t)i * 6);
    if (von_mises) von_mises[i] = rec[(size_t)i * 7 + 6];
  }
  return 0;
}
extern "C" int tlfea_t10_retrieve_principal_stress(tlfea_t10_t h, double* nodal_values, double* nodal_directions,
                                                   double* element_values, double* element_directions) {
  const std::string what = "tlfea_t10_retrieve_principal_stress";
  TRY(need_recovery(h, what));
  if (!h->rc_principal)
    return fail(what + ": the last tlfea_t10_recover_stress did not compute principal stresses (want_principal = 0)");
  if ((nodal_directions || element_directions) && !h->rc_directions)
    return fail(what + ": the last tlfea_t10_recover_stress did not compute principal directions (want_directions = 0)");
  if (nodal_values) D2H(nodal_values, h->d_rc_pn, (size_t)h->N * 4);
  if (element_values) D2H(element_values, h->d_rc_pe, (size_t)h->E * 4);
  if (nodal_directions) D2H(nodal_directions, h->d_rc_dn, (size_t)h->N * 9);
  if (element_directions) D2H(element_directions, h->d_rc_de, (size_t)h->E * 9);
  return 0;
}
extern "C" int tlfea_t10_retrieve_error_indicator(tlfea_t10_t h, double* eta2, double* n2) {
  TRY(need_recovery(h, "tlfea_t10_retrieve_error_indicator"));
  if (eta2) D2H(eta2, h->d_rc_err, (size_t)h->E);
  if (n2) D2H(n2, h->d_rc_err + h->Epad, (size_t)h->E);
  return 0;
}
extern "C" int tlfea_t10_get_error_estimate(tlfea_t10_t h, double out[4]) {
  TRY(need_recovery(h, "tlfea_t10_get_error_estimate"));
  if (!out) return fail("tlfea_t10_get_error_estimate: null output");
  std::copy_n(h->rc_tot, 4, out);
  return 0;
}
extern "C" double* tlfea_t10_recovered_stress_device_ptr(tlfea_t10_t h) {
  return h && h->kind == kT10 && h->rc_valid ? h->d_rc_nodal : nullptr;
}
// Mean duration (ms) over `reps` back-to-back launches of out[0] the element records, [1] the nodal gather from them,
// [2] the nodal gather straight from the point blocks (the form not kept), [3] the two principal launches with
// directions, [4] the error indicator, [5] its two totals launches; on the stored point stresses, which a recovery then
// follows so that the object holds the results of the form kept.
extern "C" int tlfea_t10_time_recovery_kernels(tlfea_t10_t h, int reps, double* out_ms6) {
  const std::string what = "tlfea_t10_time_recovery_kernels";
  TRY(recovery_prepare(h, what, true, 1, 1));
  if (!out_ms6) return fail(what + ": null output");
  if (reps < 1) reps = 1;
  RecoveryTable tb;
  TRY(recovery_table(h, tb));
  h->rc_valid = false;
  const int stage_of[6] = {0, 1, -1, 2, 3, 4};
  for (int k = 0; k < 6; k++)
    TRY(time_reps(h->stream, reps, &out_ms6[k], [&](int) {
      if (stage_of[k] < 0) launch_recovery_nodal_direct(h->stream, h->N, h->inc(), tb, h->d_st_pts, h->d_rc_rec, h->d_rc_nodal);
      else recovery_launch(h, tb, h->d_st_pts, 1, 1, stage_of[k]);
      return 0;
    }));
  recovery_launch(h, tb, h->d_st_pts, 1, 1, 1);  // the nodal field of the form kept, then what reads it
  for (int stage = 2; stage < 5; stage++) recovery_launch(h, tb, h->d_st_pts, 1, 1, stage);
  HIP_TRY(hipGetLastError());
  return recovery_done(h, 1, 1);
}
