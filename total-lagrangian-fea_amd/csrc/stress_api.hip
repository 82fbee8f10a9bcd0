// stress_api.hip -- C-ABI (include/tlfea_c.h) of stress and energy recovery of the data object, T10 and ANCF kinds.
#include "data_handle.h"

using namespace tlfea;

// ---- stress and energy recovery (the ANCF kinds 3f') --------------------------------------------------------
// The tlfea_t10_* and tlfea_ancf_* entry points are one implementation each.  Each family refuses the other kind of
// handle; what else differs is the set-up of the buffers (the d_st_* of the handle for both) and the three launches.
static int stress_prepare(tlfea_t10_t h, const double* d_vel, int want_points) {
  if (h && h->kind != kT10) return fail("tlfea_t10_calc_stress: T10 handles only (not an ANCF handle)");
  NEED_SETUP(h, "CalcStress.");
  if (!h->have_dndu) return fail("tlfea_t10_calc_stress: CalcDnDuPre must be called first");
  if (d_vel && h->mass_rho0 < 0.0)
    return fail("tlfea_t10_calc_stress: a velocity was given but the mass matrix is not assembled (the kinetic energy "
                "needs CalcMassMatrix)");
  if (!h->is_csr_setup) TRY(tlfea_t10_build_mass_csr_pattern(h));  // the node -> element incidence of the nodal gather
  if (!h->d_st_erec) {
    TRY(dmalloc(&h->d_st_erec, (size_t)h->E * 10));
    TRY(dmalloc(&h->d_st_contrib, (size_t)h->Epad * 4));
    TRY(dmalloc(&h->d_st_nodal, (size_t)h->N * 7));
    TRY(dmalloc(&h->d_st_part, (size_t)kStressMaxPart * 5));
    TRY(dmalloc(&h->d_st_tot, (size_t)5));
  }
  if (want_points && !h->d_st_pts) TRY(dmalloc(&h->d_st_pts, (size_t)h->E * kNQ * 6));
  return 0;
}
static void stress_launch(tlfea_t10_t h, const double* d_vel, int want_points, int stage) {
  if (stage == 0)
    launch_stress_points(h->stream, h->view(), h->mat, h->d_emat, d_vel, want_points ? h->d_st_pts : nullptr, h->d_st_erec,
                         h->d_st_contrib);
  else if (stage == 1) launch_stress_nodal(h->stream, h->N, h->inc(), h->d_st_erec, h->d_st_nodal);
  else
    launch_stress_totals(h->stream, h->E, h->Epad, h->d_st_contrib, h->N, h->inc(), h->d_mval, d_vel, h->d_st_part,
                         h->d_st_tot);
}
static int ancf_stress_prepare(tlfea_t10_t h, const double* d_vel, int want_points) {
  if (h && h->kind == kT10) return fail("tlfea_ancf_calc_stress: ANCF handles only (not a T10 handle)");
  NEED_SETUP(h, "CalcElementStress.");
  if (!h->have_dndu) return fail("tlfea_ancf_calc_stress: CalcDsDuPre must be called first");
  if (d_vel && !h->ancf_mass)
    return fail("tlfea_ancf_calc_stress: a velocity was given but the mass matrix is not assembled (the kinetic energy "
                "needs CalcMassMatrix)");
  if (!h->d_st_erec) {
    // elements of every mesh node in ascending order: node = coefficient / 4, slot 0 of local node k is row 4 k of conn
    const int E = h->E, nn = h->nn, n_nodes = h->n_nodes;
    std::vector<int> off(n_nodes + 1, 0), el((size_t)E * nn);
    for (int k = 0; k < nn; k++)
      for (int e = 0; e < E; e++) off[h->h_conn[(size_t)(4 * k) * E + e] / 4 + 1]++;
    for (int i = 0; i < n_nodes; i++) off[i + 1] += off[i];
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (int e = 0; e < E; e++)
      for (int k = 0; k < nn; k++) el[cur[h->h_conn[(size_t)(4 * k) * E + e] / 4]++] = e;
    TRY(dmalloc(&h->d_st_noff, off.size()));
    TRY(dmalloc(&h->d_st_nel, el.size()));
    HIP_TRY(hipMemcpy(h->d_st_noff, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_st_nel, el.data(), el.size() * sizeof(int), hipMemcpyHostToDevice));
    TRY(dmalloc(&h->d_st_contrib, (size_t)h->Epad * 4));
    TRY(dmalloc(&h->d_st_nodal, (size_t)n_nodes * 7));
    TRY(dmalloc(&h->d_st_part, (size_t)kStressMaxPart * 5));
    TRY(dmalloc(&h->d_st_tot, (size_t)5));
    TRY(dmalloc(&h->d_st_erec, (size_t)E * 10));
  }
  if (want_points && !h->d_st_pts) TRY(dmalloc(&h->d_st_pts, (size_t)h->E * h->Q * 6));
  return 0;
}
static void ancf_stress_launch(tlfea_t10_t h, const double* d_vel, int want_points, int stage) {
  if (stage == 0)
    launch_ancf_stress_points(h->stream, h->view(), h->mat, d_vel, want_points ? h->d_st_pts : nullptr, h->d_st_erec,
                              h->d_st_contrib);
  else if (stage == 1)
    launch_stress_node_gather(h->stream, h->n_nodes, h->d_st_noff, h->d_st_nel, h->d_st_erec, h->d_st_nodal);
  else  // the kinetic energy runs over the n_coef rows of the mass matrix
    launch_stress_totals(h->stream, h->E, h->Epad, h->d_st_contrib, h->N, h->inc(), h->d_mval, d_vel, h->d_st_part,
                         h->d_st_tot);
}

struct StressKind {
  const char* prefix;      // of the entry points' names, as the messages spell them
  bool ancf;
  const char* wrong_kind;  // what the other kind of handle is told
  const char* calc_name;   // the calc in "must be set up before"
  int (*prepare)(tlfea_t10_t, const double*, int);
  void (*launch)(tlfea_t10_t, const double*, int, int);  // stage 0 points and elements, 1 nodal record, 2 totals
  std::string name(const char* entry) const { return std::string(prefix) + entry; }
  bool refuses(tlfea_t10_t h) const { return h && (h->kind != kT10) != ancf; }
  int points(tlfea_t10_t h) const { return ancf ? h->Q : kNQ; }        // stress points per element
  int nodes(tlfea_t10_t h) const { return ancf ? h->n_nodes : h->N; }  // rows of the nodal record
};
static const StressKind kStressT10{"tlfea_t10", false, ": T10 handles only (not an ANCF handle)", "CalcStress.", stress_prepare,
                                   stress_launch};
static const StressKind kStressAncf{"tlfea_ancf", true, ": ANCF handles only (not a T10 handle)", "CalcElementStress.",
                                    ancf_stress_prepare, ancf_stress_launch};

static int stress_done(tlfea_t10_t h, int want_points) {
  HIP_TRY(hipMemcpy(h->st_tot, h->d_st_tot, 5 * sizeof(double), hipMemcpyDeviceToHost));
  h->st_valid = true;
  h->st_pts_valid = want_points != 0;
  return 0;
}
static int calc_stress(const StressKind& K, tlfea_t10_t h, const double* d_vel, int want_points) {
  TRY(K.prepare(h, d_vel, want_points));
  h->st_valid = h->st_pts_valid = false;
  for (int stage = 0; stage < 3; stage++) K.launch(h, d_vel, want_points, stage);
  HIP_TRY(hipGetLastError());
  return stress_done(h, want_points);
}
// the same with a velocity on the host (3N interleaved, or null), uploaded to a buffer of the object
static int calc_stress_host(const StressKind& K, tlfea_t10_t h, const double* vel, int want_points) {
  if (!vel) return calc_stress(K, h, nullptr, want_points);
  if (K.refuses(h)) return fail(K.name("_calc_stress") + K.wrong_kind);
  NEED_SETUP(h, K.calc_name);
  if (!h->d_st_vel) TRY(dmalloc(&h->d_st_vel, (size_t)3 * h->N));
  HIP_TRY(hipMemcpy(h->d_st_vel, vel, (size_t)3 * h->N * sizeof(double), hipMemcpyHostToDevice));
  return calc_stress(K, h, h->d_st_vel, want_points);
}
static int need_stress(const StressKind& K, tlfea_t10_t h, const std::string& what) {
  if (K.refuses(h)) return fail(what + K.wrong_kind);
  if (!h || !h->st_valid) return fail(what + ": " + K.name("_calc_stress has not been called"));
  return 0;
}
static int retrieve_point_stress(const StressKind& K, tlfea_t10_t h, double* sigma) {
  const std::string what = K.name("_retrieve_point_stress");
  TRY(need_stress(K, h, what));
  if (!h->st_pts_valid)
    return fail(what + ": the last " + K.name("_calc_stress") + " did not ask for point stresses (want_points = 0)");
  if (!sigma) return fail(what + ": null output");
  D2H(sigma, h->d_st_pts, (size_t)h->E * K.points(h) * 6);
  return 0;
}
static int retrieve_element_stress(const StressKind& K, tlfea_t10_t h, double* sigma, double* von_mises, double* psi,
                                   double* J, double* vol) {
  TRY(need_stress(K, h, K.name("_retrieve_element_stress")));
  std::vector<double> rec((size_t)h->E * 10);
  D2H(rec.data(), h->d_st_erec, rec.size());
  for (int e = 0; e < h->E; e++) {
    const double* r = &rec[(size_t)e * 10];
    if (sigma) std::copy_n(r, 6, sigma + (size_t)e * 6);
    if (von_mises) von_mises[e] = r[6];
    if (psi) psi[e] = r[7];
    if (J) J[e] = r[8];
    if (vol) vol[e] = r[9];
  }
  return 0;
}
static int retrieve_nodal_stress(const StressKind& K, tlfea_t10_t h, double* sigma, double* von_mises) {
  TRY(need_stress(K, h, K.name("_retrieve_nodal_stress")));
  const int n = K.nodes(h);
  std::vector<double> rec((size_t)n * 7);
  D2H(rec.data(), h->d_st_nodal, rec.size());
  for (int i = 0; i < n; i++) {
    if (sigma) std::copy_n(&rec[(size_t)i * 7], 6, sigma + (size_t)i * 6);
    if (von_mises) von_mises[i] = rec[(size_t)i * 7 + 6];
  }
  return 0;
}
static int get_energies(const StressKind& K, tlfea_t10_t h, double out[5]) {
  const std::string what = K.name("_get_energies");
  TRY(need_stress(K, h, what));
  if (!out) return fail(what + ": null output");
  std::copy_n(h->st_tot, 5, out);
  return 0;
}
// Mean duration (ms) over `reps` back-to-back launches of out[0] the point and element kernel, [1] the nodal record (T10:
// the nodal gather; ANCF: the mesh-node gather), [2] the two totals launches, each between one pair of events.
static int time_stress_kernels(const StressKind& K, tlfea_t10_t h, const double* d_vel, int want_points, int reps,
                               double* out_ms3) {
  TRY(K.prepare(h, d_vel, want_points));
  if (!out_ms3) return fail(K.name("_time_stress_kernels") + ": null output");
  if (reps < 1) reps = 1;
  for (int k = 0; k < 3; k++)
    TRY(time_reps(h->stream, reps, &out_ms3[k], [&](int) { K.launch(h, d_vel, want_points, k); return 0; }));
  return stress_done(h, want_points);
}

// the entry points of the two families
extern "C" int tlfea_t10_calc_stress(tlfea_t10_t h, const double* d_vel, int want_points) {
  return calc_stress(kStressT10, h, d_vel, want_points);
}
extern "C" int tlfea_t10_calc_stress_host(tlfea_t10_t h, const double* vel, int want_points) {
  return calc_stress_host(kStressT10, h, vel, want_points);
}
extern "C" int tlfea_t10_retrieve_point_stress(tlfea_t10_t h, double* sigma) { return retrieve_point_stress(kStressT10, h, sigma); }
extern "C" int tlfea_t10_retrieve_element_stress(tlfea_t10_t h, double* sigma, double* von_mises, double* psi, double* J,
                                                 double* vol) {
  return retrieve_element_stress(kStressT10, h, sigma, von_mises, psi, J, vol);
}
extern "C" int tlfea_t10_retrieve_nodal_stress(tlfea_t10_t h, double* sigma, double* von_mises) {
  return retrieve_nodal_stress(kStressT10, h, sigma, von_mises);
}
extern "C" int tlfea_t10_get_energies(tlfea_t10_t h, double out[5]) { return get_energies(kStressT10, h, out); }
extern "C" int tlfea_t10_time_stress_kernels(tlfea_t10_t h, const double* d_vel, int want_points, int reps, double* out_ms3) {
  return time_stress_kernels(kStressT10, h, d_vel, want_points, reps, out_ms3);
}
extern "C" double* tlfea_t10_nodal_stress_device_ptr(tlfea_t10_t h) { return h && h->st_valid ? h->d_st_nodal : nullptr; }

extern "C" int tlfea_ancf_calc_stress(tlfea_t10_t h, const double* d_vel, int want_points) {
  return calc_stress(kStressAncf, h, d_vel, want_points);
}
extern "C" int tlfea_ancf_calc_stress_host(tlfea_t10_t h, const double* vel, int want_points) {
  return calc_stress_host(kStressAncf, h, vel, want_points);
}
extern "C" int tlfea_ancf_retrieve_point_stress(tlfea_t10_t h, double* sigma) { return retrieve_point_stress(kStressAncf, h, sigma); }
extern "C" int tlfea_ancf_retrieve_element_stress(tlfea_t10_t h, double* sigma, double* von_mises, double* psi, double* J,
                                                  double* vol) {
  return retrieve_element_stress(kStressAncf, h, sigma, von_mises, psi, J, vol);
}
extern "C" int tlfea_ancf_retrieve_nodal_stress(tlfea_t10_t h, double* sigma, double* von_mises) {
  return retrieve_nodal_stress(kStressAncf, h, sigma, von_mises);
}
extern "C" int tlfea_ancf_get_energies(tlfea_t10_t h, double out[5]) { return get_energies(kStressAncf, h, out); }
extern "C" int tlfea_ancf_time_stress_kernels(tlfea_t10_t h, const double* d_vel, int want_points, int reps, double* out_ms3) {
  return time_stress_kernels(kStressAncf, h, d_vel, want_points, reps, out_ms3);
}
extern "C" double* tlfea_ancf_nodal_stress_device_ptr(tlfea_t10_t h) {
  return h && h->kind != kT10 && h->st_valid ? h->d_st_nodal : nullptr;
}
