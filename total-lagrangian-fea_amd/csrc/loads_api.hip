// loads_api.hip -- C-ABI (include/tlfea_c.h) of the distributed loads of the data object: body acceleration, and surface
// tractions and follower pressures on ANCF element faces and on the boundary faces of a T10 mesh (DESIGN 3h')
// through one implementation.  The gradient evaluation of the solver core reads the buffers built here.
#include "data_handle.h"
#include "ancf_load_host.h"

using namespace tlfea;

static void surface_loads_free(tlfea_t10_t h) {
  for (double** p : {&h->d_ld_tr, &h->d_ld_lbuf, &h->d_ld_tab, &h->d_ld_qw, &h->d_ld_pe}) dfree(*p);
  for (int** p : {&h->d_ld_cls, &h->d_ld_mask, &h->d_ld_fnodes, &h->d_ld_foff, &h->d_ld_fslot}) dfree(*p);
  h->h_ld_lf.clear();
  h->ld_list.clear();
  h->ld_n_trac = h->ld_n_press = 0;
}
static void loads_free(tlfea_t10_t h) {
  surface_loads_free(h);
  for (double** p : {&h->d_ld_fc, &h->d_ld_f}) dfree(*p);
  h->ld_have_a = h->ld_const_dirty = false;
  h->ld_a[0] = h->ld_a[1] = h->ld_a[2] = 0.0;
}
// the two [N][3] vectors every load needs; the total starts at zero (no gradient evaluation yet)
static int loads_alloc_common(tlfea_t10_t h) {
  if (h->d_ld_f) return 0;
  TRY(dmalloc(&h->d_ld_fc, (size_t)3 * h->N));
  TRY(dmalloc(&h->d_ld_f, (size_t)3 * h->N));
  HIP_TRY(hipMemset(h->d_ld_fc, 0, (size_t)3 * h->N * sizeof(double)));
  HIP_TRY(hipMemset(h->d_ld_f, 0, (size_t)3 * h->N * sizeof(double)));
  return 0;
}
static int t10_loads_build_pressure_scale(tlfea_t10_t h);  // on the boundary faces of a T10 mesh (DESIGN 3h')
// Traction vector [N][3] = sum over the traction loads (list order), their elements (list order), the element's
// coefficients and the face's sample points (point order) of scale t w_p S_a(p): on the host, once per change.
int tlfea::loads_build_traction(tlfea_t10_t h) {
  if (h->ld_n_trac == 0) return 0;
  if (h->kind == kT10) return t10_loads_build_traction(h);
  TRY(ancf_points_build(h));
  const int S = h->S, E = h->E, ppf = kAncfObsPoints / ancf::load_faces(S);
  std::vector<double> tr((size_t)3 * h->N, 0.0);
  for (const auto& L : h->ld_list) {
    if (L.kind != 0) continue;
    for (int e : L.elems) {
      const double* sv = &h->h_ao_sval[(size_t)h->h_ao_cls[e] * kAncfObsPoints * S];
      const double* w = &h->h_ao_w[(size_t)e * kAncfObsPoints];
      for (int a = 0; a < S; a++) {
        double ws = 0.0;
        for (int p = L.face * ppf; p < (L.face + 1) * ppf; p++) ws += w[p] * sv[(size_t)p * S + a];
        const int id = h->h_conn[(size_t)a * E + e];
        for (int c = 0; c < 3; c++) tr[3 * (size_t)id + c] += L.scale * L.value[c] * ws;
      }
    }
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->d_ld_tr, tr.data(), tr.size() * sizeof(double), hipMemcpyHostToDevice));
  h->ld_const_dirty = true;
  return 0;
}
// pe [E][faces] = -(orientation sign) x sum over the pressure loads (list order) of scale x pressure
static int loads_build_pressure_scale(tlfea_t10_t h) {
  if (h->ld_n_press == 0) return 0;
  if (h->kind == kT10) return t10_loads_build_pressure_scale(h);
  const int NF = ancf::load_faces(h->S);
  std::vector<double> pe((size_t)h->E * NF, 0.0);
  for (const auto& L : h->ld_list)
    if (L.kind == 1)
      for (int e : L.elems) pe[(size_t)e * NF + L.face] += L.scale * L.value[0];
  for (size_t k = 0; k < pe.size(); k++) pe[k] *= -ancf::load_face_sign(h->S, (int)(k % NF));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->d_ld_pe, pe.data(), pe.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

extern "C" int tlfea_clear_loads(tlfea_t10_t h) {
  NEED_SETUP(h, "clearing loads.");
  if (!h->loads_on()) return 0;
  HIP_TRY(hipDeviceSynchronize());  // launches in flight on a solver's stream may still read the buffers
  loads_free(h);
  return 0;
}
extern "C" int tlfea_set_body_acceleration(tlfea_t10_t h, const double a[3]) {
  NEED_SETUP(h, "setting a body acceleration.");
  if (h->kind != kT10 && !h->have_dndu) return fail("tlfea_set_body_acceleration: CalcDsDuPre must run first");
  if (!a) return fail("tlfea_set_body_acceleration: null acceleration");
  if (!(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2])))
    return fail("tlfea_set_body_acceleration: the acceleration must be finite");
  if (!mass_assembled(h))
    return fail("tlfea_set_body_acceleration: CalcMassMatrix must run first (the load is the mass matrix times the acceleration)");
  HIP_TRY(hipDeviceSynchronize());
  if (a[0] == 0.0 && a[1] == 0.0 && a[2] == 0.0) {  // no body force: as if never set
    h->ld_have_a = false;
    h->ld_a[0] = h->ld_a[1] = h->ld_a[2] = 0.0;
    if (!h->loads_on()) loads_free(h);
    h->ld_const_dirty = true;
    return 0;
  }
  TRY(loads_alloc_common(h));
  h->ld_have_a = true;
  std::copy(a, a + 3, h->ld_a);
  h->ld_const_dirty = true;
  return 0;
}

// ---- surface loads: one list of either kind of handle ---------------------------------------------------------------------
// What the two lists differ in: the entry point's name, what a load's index list counts (elements 0..E-1 of an ANCF mesh,
// boundary faces 0..F-1 of a T10 mesh), and the face of the element an ANCF load acts on (n_faces = 0: the entry has none).
// A T10 list travels as ANCF entries with face -1 and the face indices in `elems`.
struct LoadListKind {
  const char* who;
  const char* noun;
  int range, n_faces;
};
static int load_count_check(const char* who, int n, const void* list) {
  if (n < 0 || n > kMaxLoads)
    return fail(std::string(who) + ": n must be in 0.." + std::to_string(kMaxLoads) + ", got " + std::to_string(n));
  if (n > 0 && !list) return fail(std::string(who) + ": null list");
  return 0;
}
// Validates the entries and, when all of them pass, replaces the handle's list with them; a refused call
// leaves the handle as it was.  pressure_setup builds what the kind's pressure kernel reads, once the list is in place.
static int surface_loads_replace(tlfea_t10_t h, const LoadListKind& kd, const tlfea_surface_load* list, int n,
                                 int (*pressure_setup)(tlfea_t10_t)) {
  std::vector<tlfea_t10_s::SurfaceLoad> fresh((size_t)n);
  std::vector<char> seen;
  for (int k = 0; k < n; k++) {
    const tlfea_surface_load& L = list[k];
    const std::string who = std::string(kd.who) + ": load " + std::to_string(k) + ": ";
    if (L.kind != 0 && L.kind != 1) return fail(who + "kind must be 0 (traction) or 1 (pressure), got " + std::to_string(L.kind));
    if (kd.n_faces > 0 && (L.face < 0 || L.face >= kd.n_faces))
      return fail(who + "face " + std::to_string(L.face) + " outside 0.." + std::to_string(kd.n_faces - 1));
    for (int c = 0; c < (L.kind == 0 ? 3 : 1); c++)
      if (!std::isfinite(L.value[c])) return fail(who + "the value must be finite");
    if (!std::isfinite(L.scale)) return fail(who + "the scale must be finite");
    if (L.n_elems <= 0 || !L.elems) return fail(who + "empty " + kd.noun + " list");
    seen.assign((size_t)kd.range, 0);
    for (int i = 0; i < L.n_elems; i++) {
      const int e = L.elems[i];
      if (e < 0 || e >= kd.range)
        return fail(who + kd.noun + " " + std::to_string(e) + " outside 0.." + std::to_string(kd.range - 1));
      if (seen[e])
        return fail(who + kd.noun + " " + std::to_string(e) + " is listed twice" +
                    (kd.n_faces > 0 ? " for face " + std::to_string(L.face) : ""));
      seen[e] = 1;
    }
    fresh[k].kind = L.kind;
    fresh[k].face = L.face;
    fresh[k].scale = L.scale;
    for (int c = 0; c < 3; c++) fresh[k].value[c] = L.kind == 0 || c == 0 ? L.value[c] : 0.0;
    fresh[k].elems.assign(L.elems, L.elems + L.n_elems);
  }
  HIP_TRY(hipDeviceSynchronize());
  surface_loads_free(h);
  h->ld_const_dirty = true;
  if (n == 0) {
    if (!h->loads_on()) loads_free(h);
    return 0;
  }
  TRY(loads_alloc_common(h));
  h->ld_list.swap(fresh);
  for (const auto& L : h->ld_list) (L.kind == 0 ? h->ld_n_trac : h->ld_n_press)++;
  if (h->ld_n_trac > 0) {
    TRY(dmalloc(&h->d_ld_tr, (size_t)3 * h->N));
    TRY(loads_build_traction(h));
  }
  if (h->ld_n_press > 0) {
    TRY(pressure_setup(h));
    TRY(loads_build_pressure_scale(h));
  }
  return 0;
}
static int load_scale_update(tlfea_t10_t h, const char* who, int k, double scale) {
  NEED_SETUP(h, "updating a load scale.");
  if (k < 0 || k >= (int)h->ld_list.size())
    return fail(std::string(who) + ": index " + std::to_string(k) + " outside the " + std::to_string(h->ld_list.size()) +
                " surface loads set");
  if (!std::isfinite(scale)) return fail(std::string(who) + ": the scale must be finite");
  h->ld_list[k].scale = scale;
  return h->ld_list[k].kind == 0 ? loads_build_traction(h) : loads_build_pressure_scale(h);
}

// ANCF: the class tables of the pressure rule and the loaded faces of every element
static int ancf_pressure_setup(tlfea_t10_t h) {
  const int NF = ancf::load_faces(h->S), P = ancf::load_points(h->S), E = h->E, S = h->S;
  const ancf::PressureSetup su = ancf::pressure_setup(S, E, h->Lv, h->Wv, h->Hv, h->Binv);
  std::vector<int> mask((size_t)E, 0);
  for (const auto& L : h->ld_list)
    if (L.kind == 1)
      for (int e : L.elems) mask[e] |= 1 << L.face;
  TRY(dmalloc(&h->d_ld_cls, (size_t)E));
  TRY(dmalloc(&h->d_ld_mask, (size_t)E));
  TRY(dmalloc(&h->d_ld_tab, su.tab.size()));
  TRY(dmalloc(&h->d_ld_qw, (size_t)P));
  TRY(dmalloc(&h->d_ld_pe, (size_t)E * NF));
  TRY(dmalloc(&h->d_ld_lbuf, (size_t)E * S * 3));
  HIP_TRY(hipMemcpy(h->d_ld_cls, su.cls.data(), (size_t)E * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ld_mask, mask.data(), (size_t)E * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ld_tab, su.tab.data(), su.tab.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ld_qw, su.qw.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice));
  // zeroed once: only the rows of loaded elements are ever rewritten
  HIP_TRY(hipMemset(h->d_ld_lbuf, 0, (size_t)E * S * 3 * sizeof(double)));
  return 0;
}
extern "C" int tlfea_ancf_set_surface_loads(tlfea_t10_t h, const tlfea_surface_load* list, int n) {
  if (h && h->kind == kT10)
    return fail("tlfea_ancf_set_surface_loads: ANCF handles only (a T10 handle takes the body acceleration alone)");
  NEED_SETUP(h, "setting surface loads.");
  if (!h->have_dndu)
    return fail("tlfea_ancf_set_surface_loads: CalcDsDuPre must run first (the traction weights use the reference geometry)");
  TRY(load_count_check("tlfea_ancf_set_surface_loads", n, list));
  const LoadListKind kd{"tlfea_ancf_set_surface_loads", "element", h->E, ancf::load_faces(h->S)};
  return surface_loads_replace(h, kd, list, n, ancf_pressure_setup);
}
extern "C" int tlfea_ancf_update_load_scale(tlfea_t10_t h, int k, double scale) {
  if (h && h->kind == kT10) return fail("tlfea_ancf_update_load_scale: ANCF handles only (not a T10 handle)");
  return load_scale_update(h, "tlfea_ancf_update_load_scale", k, scale);
}

// ---- surface loads on the boundary faces of a T10 mesh (DESIGN 3h') ---------------------------------------------------------
#define NEED_T10_LOADS(h, what) \
  if ((h) && (h)->kind != kT10) return fail(std::string(what) + ": T10 handles only (not an ANCF handle)")
void tlfea::boundary_faces_build(tlfea_t10_t h) {
  if (h->bf_built) return;
  h->bf = t10load::boundary_faces(h->E, h->N, h->h_conn, h->h_X0);
  h->bf_built = true;
}
// Traction vector [N][3] = sum over the traction loads (list order), their faces (list order), the face's nodes and the
// points of the rule (point order) of scale t w_q N_a(q) |X_xi x X_eta|(q): on the host, once per change.
int tlfea::t10_loads_build_traction(tlfea_t10_t h) {
  std::vector<double> tr((size_t)3 * h->N, 0.0);
  for (const auto& L : h->ld_list) {
    if (L.kind != 0) continue;
    for (int k : L.elems) {
      const int* nd = &h->bf.nodes[(size_t)k * 6];
      double w[6];
      t10load::traction_weights(nd, h->N, h->h_X0, w);
      for (int a = 0; a < 6; a++)
        for (int c = 0; c < 3; c++) tr[3 * (size_t)nd[a] + c] += L.scale * L.value[c] * w[a];
    }
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->d_ld_tr, tr.data(), tr.size() * sizeof(double), hipMemcpyHostToDevice));
  h->ld_const_dirty = true;
  return 0;
}
// pe [loaded faces] = -(sum over the pressure loads (list order) of scale x pressure): the nodes are ordered outward
static int t10_loads_build_pressure_scale(tlfea_t10_t h) {
  std::vector<double> pf((size_t)h->bf.count(), 0.0);
  for (const auto& L : h->ld_list)
    if (L.kind == 1)
      for (int k : L.elems) pf[k] += L.scale * L.value[0];
  std::vector<double> pe(h->h_ld_lf.size());
  for (size_t i = 0; i < pe.size(); i++) pe[i] = -pf[h->h_ld_lf[i]];
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h->d_ld_pe, pe.data(), pe.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

extern "C" int tlfea_t10_get_boundary_faces(tlfea_t10_t h, int* n_faces, int* elem, int* local_face, int* nodes) {
  NEED_T10_LOADS(h, "tlfea_t10_get_boundary_faces");
  NEED_SETUP(h, "reading boundary faces.");
  if (!n_faces) return fail("tlfea_t10_get_boundary_faces: null count");
  boundary_faces_build(h);
  *n_faces = h->bf.count();
  if (elem) std::copy(h->bf.elem.begin(), h->bf.elem.end(), elem);
  if (local_face) std::copy(h->bf.local_face.begin(), h->bf.local_face.end(), local_face);
  if (nodes) std::copy(h->bf.nodes.begin(), h->bf.nodes.end(), nodes);
  return 0;
}
// T10: the loaded faces, ascending; the rows of a node in ascending (loaded face, local node) order
static int t10_pressure_setup(tlfea_t10_t h) {
  const int F = h->bf.count();
  std::vector<char> loaded((size_t)F, 0);
  for (const auto& L : h->ld_list)
    if (L.kind == 1)
      for (int f : L.elems) loaded[f] = 1;
  for (int f = 0; f < F; f++)
    if (loaded[f]) h->h_ld_lf.push_back(f);
  const size_t nlf = h->h_ld_lf.size();
  std::vector<int> fnodes(nlf * 6), off((size_t)h->N + 1, 0), slot(nlf * 6);
  for (size_t i = 0; i < nlf; i++)
    for (int a = 0; a < 6; a++) {
      fnodes[i * 6 + a] = h->bf.nodes[(size_t)h->h_ld_lf[i] * 6 + a];
      off[fnodes[i * 6 + a] + 1]++;
    }
  for (int i = 0; i < h->N; i++) off[i + 1] += off[i];
  std::vector<int> fill(off.begin(), off.end() - 1);
  for (size_t r = 0; r < nlf * 6; r++) slot[fill[fnodes[r]]++] = (int)r;
  TRY(dmalloc(&h->d_ld_fnodes, nlf * 6));
  TRY(dmalloc(&h->d_ld_foff, (size_t)h->N + 1));
  TRY(dmalloc(&h->d_ld_fslot, nlf * 6));
  TRY(dmalloc(&h->d_ld_pe, nlf));
  TRY(dmalloc(&h->d_ld_lbuf, nlf * 18));
  HIP_TRY(hipMemcpy(h->d_ld_fnodes, fnodes.data(), fnodes.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ld_foff, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_ld_fslot, slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(h->d_ld_lbuf, 0, nlf * 18 * sizeof(double)));
  return 0;
}
extern "C" int tlfea_t10_set_surface_loads(tlfea_t10_t h, const tlfea_t10_surface_load* list, int n) {
  NEED_T10_LOADS(h, "tlfea_t10_set_surface_loads");
  NEED_SETUP(h, "setting surface loads.");
  TRY(load_count_check("tlfea_t10_set_surface_loads", n, list));
  boundary_faces_build(h);
  const LoadListKind kd{"tlfea_t10_set_surface_loads", "face", h->bf.count(), 0};
  std::vector<tlfea_surface_load> in((size_t)n);
  for (int k = 0; k < n; k++) {
    in[k].kind = list[k].kind;
    in[k].face = -1;
    std::copy(list[k].value, list[k].value + 3, in[k].value);
    in[k].scale = list[k].scale;
    in[k].elems = list[k].faces;
    in[k].n_elems = list[k].n_faces;
  }
  return surface_loads_replace(h, kd, in.data(), n, t10_pressure_setup);
}
extern "C" int tlfea_t10_update_load_scale(tlfea_t10_t h, int k, double scale) {
  NEED_T10_LOADS(h, "tlfea_t10_update_load_scale");
  return load_scale_update(h, "tlfea_t10_update_load_scale", k, scale);
}

extern "C" int tlfea_get_load_forces(tlfea_t10_t h, double* f) {
  NEED_SETUP(h, "reading load forces.");
  if (!f) return fail("tlfea_get_load_forces: null output");
  if (!h->loads_on()) {
    std::fill(f, f + 3 * (size_t)h->N, 0.0);
    return 0;
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(f, h->d_ld_f, 3 * (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int tlfea_get_load_resultant(tlfea_t10_t h, double out[3]) {
  NEED_SETUP(h, "reading the load resultant.");
  if (!out) return fail("tlfea_get_load_resultant: null output");
  std::vector<double> f((size_t)3 * h->N);
  TRY(tlfea_get_load_forces(h, f.data()));
  const int stride = h->kind == kT10 ? 1 : 4;  // the position coefficients, ascending
  out[0] = out[1] = out[2] = 0.0;
  for (int i = 0; i < h->N; i += stride)
    for (int c = 0; c < 3; c++) out[c] += f[3 * (size_t)i + c];
  return 0;
}
