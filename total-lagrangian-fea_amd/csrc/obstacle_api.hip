// obstacle_api.hip -- C-ABI (include/tlfea_c.h) of rigid obstacles of the data object: analytic ones on T10 and ANCF
// handles, field obstacles (signed-distance grids) on any handle, and the signed-distance grid of a triangle surface.
#include "ancf_obstacle_host.h"
#include "data_handle.h"
#include "field_obstacle_host.h"
#include "obstacle_host.h"

using namespace tlfea;

// ---- rigid obstacles ---------------------------------------------------------------------------------------------------
static void surface_build(tlfea_t10_t h) {
  if (!h->h_surf_w.empty()) return;
  h->h_surf_w = t10_surface_weights(h->E, h->N, h->h_conn, h->h_X0);
  h->h_surf.clear();
  for (int i = 0; i < h->N; i++)
    if (h->h_surf_w[i] > 0.0) h->h_surf.push_back(i);
}
// The reference geometry moved: the weights are reference areas.  The connectivity and with it the set of surface nodes
// stay, so the node list and every node-owned buffer keep their size; only the weights are replaced.
int tlfea::t10_surface_refresh(tlfea_t10_t h) {
  if (h->h_surf_w.empty()) return 0;  // never built: the first use builds them from the new geometry
  const std::vector<int> nodes = h->h_surf;
  h->h_surf_w.clear();
  surface_build(h);
  if (h->h_surf != nodes) return fail("tlfea_t10_set_reference_positions: the set of surface nodes changed (a boundary face of zero area)");
  if (h->d_ob_w && !h->h_surf.empty()) {
    std::vector<double> w(h->h_surf.size());
    for (size_t k = 0; k < w.size(); k++) w[k] = h->h_surf_w[h->h_surf[k]];
    HIP_TRY(hipMemcpy(h->d_ob_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  return 0;
}
static void obstacles_free(tlfea_t10_t h) {
  for (double** p : {&h->d_ob_w, &h->d_ob_f, &h->d_ob_blk, &h->d_ob_fk, &h->d_ob_res}) dfree(*p);
  dfree(h->d_ob_node);
  h->ob_fk_cap = 0;
  h->obs.n = h->ob_na = 0;
}
// The node-owned buffers for a list of n obstacles (analytic and field together): allocated on first use, fk grown, all
// zeroed -- no forces before the first gradient evaluation.
static int obstacle_buffers(tlfea_t10_t h, int n) {
  surface_build(h);
  const int ns = (int)h->h_surf.size();
  if (!h->d_ob_node) {
    std::vector<double> w(ns);
    for (int k = 0; k < ns; k++) w[k] = h->h_surf_w[h->h_surf[k]];
    TRY(dmalloc(&h->d_ob_node, (size_t)ns));
    TRY(dmalloc(&h->d_ob_w, (size_t)ns));
    TRY(dmalloc(&h->d_ob_f, (size_t)3 * ns));
    TRY(dmalloc(&h->d_ob_blk, (size_t)6 * ns));
    TRY(dmalloc(&h->d_ob_res, (size_t)4 * kMaxObstacles));
    if (ns) {
      HIP_TRY(hipMemcpy(h->d_ob_node, h->h_surf.data(), (size_t)ns * sizeof(int), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(h->d_ob_w, w.data(), (size_t)ns * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  if (h->ob_fk_cap < n) {
    dfree(h->d_ob_fk);
    TRY(dmalloc(&h->d_ob_fk, (size_t)4 * n * ns));
    h->ob_fk_cap = n;
  }
  HIP_TRY(hipMemset(h->d_ob_f, 0, (size_t)std::max(1, 3 * ns) * sizeof(double)));
  HIP_TRY(hipMemset(h->d_ob_blk, 0, (size_t)std::max(1, 6 * ns) * sizeof(double)));
  HIP_TRY(hipMemset(h->d_ob_fk, 0, (size_t)std::max(1, 4 * n * ns) * sizeof(double)));
  return 0;
}
// The list the kernels see: the analytic obstacles `a`, then the fields of h->fld in their order.
static void obstacle_list_set(tlfea_t10_t h, const std::vector<ObstacleDev>& a) {
  h->ob_na = (int)a.size();
  for (int k = 0; k < h->ob_na; k++) h->obs.o[k] = a[k];
  for (size_t k = 0; k < h->fld.size(); k++) h->obs.o[h->ob_na + k] = field_obstacle_dev(h->fld[k], h->d_fld + k);
  h->obs.n = h->ob_na + (int)h->fld.size();
}
static std::vector<ObstacleDev> obstacle_list_analytic(tlfea_t10_t h) {
  return std::vector<ObstacleDev>(h->obs.o, h->obs.o + h->ob_na);
}
static std::string obstacle_overflow(int n_analytic, int n_field) {
  return std::to_string(n_analytic) + " analytic and " + std::to_string(n_field) + " field obstacles exceed the " +
         std::to_string(kMaxObstacles) + " an object can hold";
}
// The tlfea_t10_* calls on the analytic list refuse an ANCF handle: set_obstacles always (`strict`), the others only while
// the handle holds a list -- an ANCF object's list belongs to the tlfea_ancf_* calls (DESIGN 3e').  `doing` completes
// "must be set up before".
static int t10_obs_need(tlfea_t10_t h, const std::string& what, const char* doing, bool strict) {
  if (h && h->kind != kT10 && (strict || h->obs.n > 0)) return fail(what + ": T10 handles only (not an ANCF handle)");
  NEED_SETUP(h, doing);
  return 0;
}

// ---- rigid obstacles on the ANCF kinds (DESIGN 3e') ------------------------------------------------------------------------
static int ancf_obs_need(tlfea_t10_t h, const std::string& what, const char* = nullptr, bool = false) {
  if (h && h->kind == kT10) return fail(what + ": ANCF handles only (not a T10 handle)");
  NEED_SETUP(h, what + ".");
  if (!h->have_dndu) return fail(what + ": CalcDsDuPre must run first (the point weights use the reference geometry)");
  return 0;
}
// Weights and shape tables from the reference coefficients (x12_jac = d_xt).  Built by the first SetRigidObstacles /
// GetSurfacePointWeights after a CalcDsDuPre, which drops the cache.  d_xt is also the constraint target: targets moved
// (UpdateConstraintTargets) between CalcDsDuPre and that first use would be taken for the reference, as they would by a
// second CalcDsDuPre itself.
int tlfea::ancf_points_build(tlfea_t10_t h) {
  if (!h->h_ao_w.empty()) return 0;
  const size_t N = h->N;
  std::vector<double> xj(N), yj(N), zj(N);
  HIP_TRY(hipMemcpy(xj.data(), h->d_xt, N * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(yj.data(), h->d_yt, N * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(zj.data(), h->d_zt, N * sizeof(double), hipMemcpyDeviceToHost));
  ancf::ObstacleSetup su =
      ancf::obstacle_setup(h->S, h->E, h->h_conn, h->Lv, h->Wv, h->Hv, h->Binv, xj.data(), yj.data(), zj.data());
  h->h_ao_w.swap(su.w);
  h->h_ao_cls.swap(su.cls);
  h->h_ao_sval.swap(su.sval);
  return 0;
}
static void ancf_obstacles_free(tlfea_t10_t h) {
  for (double** p : {&h->d_ao_sval, &h->d_ao_w, &h->d_ao_cbuf, &h->d_ao_blk, &h->d_ao_fk, &h->d_ao_fc, &h->d_ao_pts,
                     &h->d_ob_res}) dfree(*p);
  for (int** p : {&h->d_ao_cls, &h->d_ao_touched}) dfree(*p);
  h->ob_fk_cap = 0;
  h->obs.n = h->ob_na = 0;
}
// The element-owned buffers for a list of n obstacles (analytic and field together): allocated on first use, fk grown,
// zeroed -- no forces and no touched element before the first gradient evaluation.
static int ancf_obstacle_buffers(tlfea_t10_t h, int n) {
  TRY(ancf_points_build(h));
  const size_t E = h->E, S = h->S, P = kAncfObsPoints;
  if (!h->d_ao_w) {
    TRY(dmalloc(&h->d_ao_cls, E));
    TRY(dmalloc(&h->d_ao_touched, E));
    TRY(dmalloc(&h->d_ao_sval, h->h_ao_sval.size()));
    TRY(dmalloc(&h->d_ao_w, E * P));
    TRY(dmalloc(&h->d_ao_cbuf, E * S * 3));
    TRY(dmalloc(&h->d_ao_blk, E * P * 6));
    TRY(dmalloc(&h->d_ao_fc, (size_t)3 * h->N));
    TRY(dmalloc(&h->d_ob_res, (size_t)4 * kMaxObstacles));
    HIP_TRY(hipMemcpy(h->d_ao_cls, h->h_ao_cls.data(), E * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_ao_sval, h->h_ao_sval.data(), h->h_ao_sval.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_ao_w, h->h_ao_w.data(), E * P * sizeof(double), hipMemcpyHostToDevice));
  }
  if (h->ob_fk_cap < n) {
    dfree(h->d_ao_fk);
    TRY(dmalloc(&h->d_ao_fk, (size_t)4 * n * E));
    h->ob_fk_cap = n;
  }
  HIP_TRY(hipMemset(h->d_ao_touched, 0, E * sizeof(int)));
  HIP_TRY(hipMemset(h->d_ao_cbuf, 0, E * S * 3 * sizeof(double)));
  HIP_TRY(hipMemset(h->d_ao_fc, 0, (size_t)3 * h->N * sizeof(double)));
  HIP_TRY(hipMemset(h->d_ao_fk, 0, (size_t)4 * n * E * sizeof(double)));
  return 0;
}

// ---- the analytic list, either kind of handle ----------------------------------------------------------------------------
// One implementation each of clear, set, update and get_resultant.  What a kind brings: the prefix of its entry points'
// names, its precondition, its buffers, and where get_resultant finds the per-obstacle shares (T10: one row per surface
// node; ANCF: the elements' shares, element order).
struct ObsHandleKind {
  const char* prefix;
  int (*need)(tlfea_t10_t, const std::string& what, const char* doing, bool strict);
  int (*buffers)(tlfea_t10_t, int);
  void (*free_all)(tlfea_t10_t);
  int (*res_rows)(tlfea_t10_t);
  double* (*res_shares)(tlfea_t10_t);
  std::string name(const char* entry) const { return std::string(prefix) + entry; }
};
static const ObsHandleKind kObsT10{"tlfea_t10", t10_obs_need, obstacle_buffers, obstacles_free,
                                  [](tlfea_t10_t h) { return (int)h->h_surf.size(); }, [](tlfea_t10_t h) { return h->d_ob_fk; }};
static const ObsHandleKind kObsAncf{"tlfea_ancf", ancf_obs_need, ancf_obstacle_buffers, ancf_obstacles_free,
                                   [](tlfea_t10_t h) { return h->E; }, [](tlfea_t10_t h) { return h->d_ao_fk; }};

static int clear_obstacles(const ObsHandleKind& K, tlfea_t10_t h) {
  TRY(K.need(h, K.name("_clear_obstacles"), "clearing obstacles.", false));
  if (h->ob_na == 0) return 0;
  HIP_TRY(hipDeviceSynchronize());  // launches in flight on a solver's stream may still read the buffers
  if (h->fld.empty()) {
    K.free_all(h);
  } else {  // the field list stays (DESIGN 3e'')
    TRY(K.buffers(h, (int)h->fld.size()));
    obstacle_list_set(h, {});
  }
  return 0;
}
static int set_obstacles(const ObsHandleKind& K, tlfea_t10_t h, const tlfea_obstacle* list, int n) {
  const std::string what = K.name("_set_obstacles");
  TRY(K.need(h, what, "setting obstacles.", true));
  if (n < 0 || n > kMaxObstacles)
    return fail(what + ": n must be in 0.." + std::to_string(kMaxObstacles) + ", got " + std::to_string(n));
  if (n > 0 && !list) return fail(what + ": null list");
  for (int k = 0; k < n; k++) {
    const std::string why = obstacle_check(list[k]);
    if (!why.empty()) return fail(what + ": obstacle " + std::to_string(k) + ": " + why);
  }
  if (n + (int)h->fld.size() > kMaxObstacles) return fail(what + ": " + obstacle_overflow(n, (int)h->fld.size()));
  if (n == 0) return clear_obstacles(K, h);
  HIP_TRY(hipDeviceSynchronize());
  TRY(K.buffers(h, n + (int)h->fld.size()));
  std::vector<ObstacleDev> a(n);
  for (int k = 0; k < n; k++) a[k] = obstacle_dev(list[k]);
  obstacle_list_set(h, a);
  return 0;
}
static int update_obstacle(const ObsHandleKind& K, tlfea_t10_t h, int k, const tlfea_obstacle* o) {
  const std::string what = K.name("_update_obstacle");
  TRY(K.need(h, what, "updating an obstacle.", false));
  if (k < 0 || k >= h->ob_na)
    return fail(what + ": index " + std::to_string(k) + " outside the " + std::to_string(h->ob_na) + " obstacles set");
  if (!o) return fail(what + ": null obstacle");
  const std::string why = obstacle_check(*o);
  if (!why.empty()) return fail(what + ": obstacle " + std::to_string(k) + ": " + why);
  h->obs.o[k] = obstacle_dev(*o);  // a kernel argument: launches already queued keep the old value
  return 0;
}
static int get_obstacle_resultant(const ObsHandleKind& K, tlfea_t10_t h, int k, double out[4]) {
  const std::string what = K.name("_get_obstacle_resultant");
  TRY(K.need(h, what, "reading an obstacle resultant.", false));
  if (!out) return fail(what + ": null output");
  if (k < 0 || k >= h->ob_na)
    return fail(what + ": index " + std::to_string(k) + " outside the " + std::to_string(h->ob_na) + " obstacles set");
  HIP_TRY(hipDeviceSynchronize());
  launch_obstacle_resultant(h->stream, K.res_rows(h), h->obs.n, K.res_shares(h), h->d_ob_res);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, h->d_ob_res + 4 * k, 4 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int tlfea_t10_clear_obstacles(tlfea_t10_t h) { return clear_obstacles(kObsT10, h); }
extern "C" int tlfea_t10_set_obstacles(tlfea_t10_t h, const tlfea_obstacle* list, int n) { return set_obstacles(kObsT10, h, list, n); }
extern "C" int tlfea_t10_update_obstacle(tlfea_t10_t h, int k, const tlfea_obstacle* o) { return update_obstacle(kObsT10, h, k, o); }
extern "C" int tlfea_t10_get_obstacle_resultant(tlfea_t10_t h, int k, double out[4]) {
  return get_obstacle_resultant(kObsT10, h, k, out);
}
extern "C" int tlfea_ancf_clear_obstacles(tlfea_t10_t h) { return clear_obstacles(kObsAncf, h); }
extern "C" int tlfea_ancf_set_obstacles(tlfea_t10_t h, const tlfea_obstacle* list, int n) { return set_obstacles(kObsAncf, h, list, n); }
extern "C" int tlfea_ancf_update_obstacle(tlfea_t10_t h, int k, const tlfea_obstacle* o) { return update_obstacle(kObsAncf, h, k, o); }
extern "C" int tlfea_ancf_get_obstacle_resultant(tlfea_t10_t h, int k, double out[4]) {
  return get_obstacle_resultant(kObsAncf, h, k, out);
}

// ---- what only one kind has ---------------------------------------------------------------------------------------------
extern "C" int tlfea_t10_get_obstacle_forces(tlfea_t10_t h, double* f) {
  TRY(t10_obs_need(h, "tlfea_t10_get_obstacle_forces", "reading obstacle forces.", false));
  if (!f) return fail("tlfea_t10_get_obstacle_forces: null output");
  std::fill(f, f + 3 * (size_t)h->N, 0.0);
  if (h->obs.n == 0) return 0;
  const size_t ns = h->h_surf.size();
  std::vector<double> fs(3 * ns);
  HIP_TRY(hipDeviceSynchronize());
  if (ns) HIP_TRY(hipMemcpy(fs.data(), h->d_ob_f, 3 * ns * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < ns; k++)
    for (int c = 0; c < 3; c++) f[3 * (size_t)h->h_surf[k] + c] = fs[3 * k + c];
  return 0;
}
extern "C" int tlfea_t10_get_surface_weights(tlfea_t10_t h, double* w) {
  if (h && h->kind != kT10) return fail("tlfea_t10_get_surface_weights: T10 handles only (not an ANCF handle)");
  NEED_SETUP(h, "reading surface weights.");
  if (!w) return fail("tlfea_t10_get_surface_weights: null output");
  surface_build(h);
  std::copy(h->h_surf_w.begin(), h->h_surf_w.end(), w);
  return 0;
}
extern "C" int tlfea_ancf_get_obstacle_forces(tlfea_t10_t h, double* f) {
  TRY(ancf_obs_need(h, "tlfea_ancf_get_obstacle_forces"));
  if (!f) return fail("tlfea_ancf_get_obstacle_forces: null output");
  if (h->obs.n == 0) {
    std::fill(f, f + 3 * (size_t)h->N, 0.0);
    return 0;
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(f, h->d_ao_fc, 3 * (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int tlfea_ancf_get_surface_points(tlfea_t10_t h, double* w) {
  TRY(ancf_obs_need(h, "tlfea_ancf_get_surface_points"));
  if (!w) return fail("tlfea_ancf_get_surface_points: null output");
  TRY(ancf_points_build(h));
  std::copy(h->h_ao_w.begin(), h->h_ao_w.end(), w);
  return 0;
}
extern "C" int tlfea_ancf_retrieve_contact_points(tlfea_t10_t h, double* out) {
  TRY(ancf_obs_need(h, "tlfea_ancf_retrieve_contact_points"));
  if (!out) return fail("tlfea_ancf_retrieve_contact_points: null output");
  if (h->obs.n == 0) return fail("tlfea_ancf_retrieve_contact_points: no obstacles are set");
  const size_t n = (size_t)h->E * kAncfObsPoints * 5;
  HIP_TRY(hipDeviceSynchronize());
  if (!h->d_ao_pts) TRY(dmalloc(&h->d_ao_pts, n));
  launch_ancf_obstacle_footprint(h->stream, ancf_obs_view(h), h->obs, h->d_x, h->d_y, h->d_z, h->d_ao_pts);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, h->d_ao_pts, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// ---- field obstacles (DESIGN 3e''), any handle ---------------------------------------------------------------------------
#define NEED_FIELD_OBS(h, what)                                                                              \
  NEED_SETUP(h, what ".");                                                                                   \
  if ((h)->kind != kT10 && !(h)->have_dndu)                                                                  \
  return fail(std::string(what) + ": CalcDsDuPre must run first (the point weights use the reference geometry)")
static void field_storage_free(tlfea_t10_t h) {
  for (double* p : h->d_fld_V)
    if (p) (void)hipFree(p);
  h->d_fld_V.clear();
  h->fld.clear();
}
extern "C" int tlfea_clear_field_obstacles(tlfea_t10_t h) {
  NEED_FIELD_OBS(h, "tlfea_clear_field_obstacles");
  if (h->fld.empty()) return 0;
  HIP_TRY(hipDeviceSynchronize());  // launches in flight on a solver's stream may still read the samples
  field_storage_free(h);
  if (h->ob_na == 0) {
    if (h->kind == kT10)
      obstacles_free(h);
    else
      ancf_obstacles_free(h);
    dfree(h->d_fld);
  } else {  // the analytic list stays
    TRY(h->kind == kT10 ? obstacle_buffers(h, h->ob_na) : ancf_obstacle_buffers(h, h->ob_na));
    obstacle_list_set(h, obstacle_list_analytic(h));
  }
  return 0;
}
extern "C" int tlfea_set_field_obstacles(tlfea_t10_t h, const tlfea_field_obstacle* list, const double* const* values,
                                         int n) {
  NEED_FIELD_OBS(h, "tlfea_set_field_obstacles");
  if (n < 0 || n > kMaxObstacles)
    return fail("tlfea_set_field_obstacles: n must be in 0.." + std::to_string(kMaxObstacles) + ", got " + std::to_string(n));
  if (n > 0 && !list) return fail("tlfea_set_field_obstacles: null list");
  if (n > 0 && !values) return fail("tlfea_set_field_obstacles: null sample pointer");
  for (int k = 0; k < n; k++) {
    if (!values[k]) return fail("tlfea_set_field_obstacles: field " + std::to_string(k) + ": null sample pointer");
    std::string why = field_params_check(list[k]);
    if (why.empty()) why = field_values_check(list[k], values[k]);
    if (!why.empty()) return fail("tlfea_set_field_obstacles: field " + std::to_string(k) + ": " + why);
  }
  if (n + h->ob_na > kMaxObstacles) return fail("tlfea_set_field_obstacles: " + obstacle_overflow(h->ob_na, n));
  if (n == 0) return tlfea_clear_field_obstacles(h);
  HIP_TRY(hipDeviceSynchronize());
  // the new samples are allocated and copied first and swapped in only when all of that has succeeded: a failure leaves
  // the previous list as it was
  std::vector<double*> fresh;
  auto drop = [&](int r) {
    for (double* p : fresh) (void)hipFree(p);
    return r;
  };
  FieldDev desc[kMaxObstacles] = {};
  for (int k = 0; k < n; k++) {
    const size_t ns = (size_t)list[k].nx * list[k].ny * list[k].nz;
    double* d_V = nullptr;
    if (int r = dmalloc(&d_V, ns)) return drop(r);
    fresh.push_back(d_V);
    if (hipMemcpy(d_V, values[k], ns * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      return drop(fail("tlfea_set_field_obstacles: copying the samples of field " + std::to_string(k) + " failed"));
    desc[k] = field_dev(list[k], d_V);
  }
  // the descriptors go to a fresh device array: the one in use, which the list entries point into, is untouched until
  // every allocation and copy has succeeded
  FieldDev* d_fld_new = nullptr;
  if (int r = dmalloc(&d_fld_new, (size_t)kMaxObstacles)) return drop(r);
  if (hipMemcpy(d_fld_new, desc, (size_t)n * sizeof(FieldDev), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d_fld_new);
    return drop(fail("tlfea_set_field_obstacles: copying the descriptors failed"));
  }
  if (int r = h->kind == kT10 ? obstacle_buffers(h, h->ob_na + n) : ancf_obstacle_buffers(h, h->ob_na + n)) {
    (void)hipFree(d_fld_new);  // the shared buffers may have been re-zeroed: no forces until the next evaluation
    return drop(r);
  }
  if (h->d_fld) (void)hipFree(h->d_fld);
  h->d_fld = d_fld_new;
  const std::vector<ObstacleDev> analytic = obstacle_list_analytic(h);
  field_storage_free(h);
  h->d_fld_V.swap(fresh);
  std::copy(desc, desc + n, h->h_fld);
  h->fld.assign(list, list + n);
  obstacle_list_set(h, analytic);
  return 0;
}
extern "C" int tlfea_update_field_obstacle(tlfea_t10_t h, int k, const tlfea_field_obstacle* o) {
  NEED_FIELD_OBS(h, "tlfea_update_field_obstacle");
  if (k < 0 || k >= (int)h->fld.size())
    return fail("tlfea_update_field_obstacle: index " + std::to_string(k) + " outside the " +
                std::to_string(h->fld.size()) + " field obstacles set");
  if (!o) return fail("tlfea_update_field_obstacle: null obstacle");
  const std::string why = field_params_check(*o);
  if (!why.empty()) return fail("tlfea_update_field_obstacle: field " + std::to_string(k) + ": " + why);
  const tlfea_field_obstacle& old = h->fld[k];
  if (o->nx != old.nx || o->ny != old.ny || o->nz != old.nz)
    return fail("tlfea_update_field_obstacle: field " + std::to_string(k) + ": the grid is " + std::to_string(o->nx) +
                " x " + std::to_string(o->ny) + " x " + std::to_string(o->nz) + ", the stored one " +
                std::to_string(old.nx) + " x " + std::to_string(old.ny) + " x " + std::to_string(old.nz));
  // the descriptor: a small copy ordered on the object's stream (the solvers' streams synchronise with it); position,
  // velocity and the contact parameters are kernel arguments: launches already queued keep the old values
  h->h_fld[k] = field_dev(*o, h->d_fld_V[k]);
  HIP_TRY(hipMemcpyAsync(h->d_fld + k, &h->h_fld[k], sizeof(FieldDev), hipMemcpyHostToDevice, h->stream));
  h->fld[k] = *o;
  h->obs.o[h->ob_na + k] = field_obstacle_dev(*o, h->d_fld + k);
  return 0;
}
extern "C" int tlfea_get_field_obstacle_resultant(tlfea_t10_t h, int k, double out[4]) {
  NEED_FIELD_OBS(h, "tlfea_get_field_obstacle_resultant");
  if (!out) return fail("tlfea_get_field_obstacle_resultant: null output");
  if (k < 0 || k >= (int)h->fld.size())
    return fail("tlfea_get_field_obstacle_resultant: index " + std::to_string(k) + " outside the " +
                std::to_string(h->fld.size()) + " field obstacles set");
  HIP_TRY(hipDeviceSynchronize());
  if (h->kind == kT10)
    launch_obstacle_resultant(h->stream, (int)h->h_surf.size(), h->obs.n, h->d_ob_fk, h->d_ob_res);
  else
    launch_obstacle_resultant(h->stream, h->E, h->obs.n, h->d_ao_fk, h->d_ob_res);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, h->d_ob_res + 4 * (h->ob_na + k), 4 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
// Launches of at most kSdfPairsPerLaunch (sample, triangle) pairs each, so that none is long-running (DESIGN 3e'').
constexpr long long kSdfPairsPerLaunch = 1ll << 32;
constexpr int kSdfMaxTriangles = 1 << 24;  // 256 samples x 2^24 triangles = the bound: every launch holds a whole block
extern "C" int tlfea_sdf_from_triangles(const double* verts, int n_verts, const int* tris, int n_tris, int nx, int ny,
                                        int nz, const double origin[3], double spacing, double* values) {
  if (!verts || !tris || !origin || !values) return fail("tlfea_sdf_from_triangles: null argument");
  if (nx < 1 || ny < 1 || nz < 1) return fail("tlfea_sdf_from_triangles: the grid needs at least one sample per axis");
  if ((long long)nx * ny * nz > kMaxFieldSamples) return fail("tlfea_sdf_from_triangles: more than 2^27 samples");
  if (!(spacing > 0.0) || !std::isfinite(spacing)) return fail("tlfea_sdf_from_triangles: spacing must be > 0");
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(origin[c])) return fail("tlfea_sdf_from_triangles: non-finite origin");
  if (n_verts < 0 || n_tris < 0) return fail("tlfea_sdf_from_triangles: negative count");
  if (n_tris > kSdfMaxTriangles)  // a launch of one block of samples would exceed the pair bound
    return fail("tlfea_sdf_from_triangles: more than 2^24 triangles");
  const std::string why = surface_check(verts, n_verts, tris, n_tris);
  if (!why.empty()) return fail("tlfea_sdf_from_triangles: " + why);
  std::vector<double> tri((size_t)9 * n_tris);
  for (int t = 0; t < n_tris; t++)
    for (int c = 0; c < 3; c++)
      for (int a = 0; a < 3; a++) tri[(size_t)9 * t + 3 * c + a] = verts[3 * (size_t)tris[3 * t + c] + a];
  const long long ns = (long long)nx * ny * nz;
  double *d_tri = nullptr, *d_out = nullptr;
  TRY(dmalloc(&d_tri, tri.size()));
  if (int r = dmalloc(&d_out, (size_t)ns)) {
    (void)hipFree(d_tri);
    return r;
  }
  hipError_t e = hipMemcpy(d_tri, tri.data(), tri.size() * sizeof(double), hipMemcpyHostToDevice);
  const long long per = std::max(256ll, kSdfPairsPerLaunch / n_tris / 256 * 256);
  for (long long first = 0; first < ns && e == hipSuccess; first += per) {
    launch_sdf_from_triangles(nullptr, d_tri, n_tris, nx, ny, origin, spacing, first, std::min(per, ns - first), d_out);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  }
  if (e == hipSuccess) e = hipMemcpy(values, d_out, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d_tri);
  (void)hipFree(d_out);
  HIP_TRY(e);
  return 0;
}
