// data_api.hip -- C-ABI (include/tlfea_c.h) of the data object behind tlfea_t10_t, any element kind: buffer ownership,
// materials, fixed nodes and linear constraints, the shape-function tables, the mass pattern and matrix, the element-level
// stress and internal force, the read-backs and the VTK writer.
#include <fstream>

#include "ancf_host.h"
#include "data_handle.h"

using namespace tlfea;

static int alloc_common(tlfea_t10_t h) {
  const size_t E = h->E, N = h->N, S = h->S, Q = h->Q;
  h->Epad = (h->E + 63) / 64 * 64;
  TRY(dmalloc(&h->d_conn, E * S));
  TRY(dmalloc(&h->d_x, N)); TRY(dmalloc(&h->d_y, N)); TRY(dmalloc(&h->d_z, N));
  TRY(dmalloc(&h->d_xt, N)); TRY(dmalloc(&h->d_yt, N)); TRY(dmalloc(&h->d_zt, N));
  TRY(dmalloc(&h->d_qx, kNQ)); TRY(dmalloc(&h->d_qy, kNQ)); TRY(dmalloc(&h->d_qz, kNQ));
  TRY(dmalloc(&h->d_gradN, E * Q * 3 * S));
  TRY(dmalloc(&h->d_gradN_t, (size_t)h->Epad * Q * 3 * S));
  TRY(dmalloc(&h->d_detJ, E * Q));
  TRY(dmalloc(&h->d_fbuf, E * 3 * S));
  TRY(dmalloc(&h->d_fint, 3 * N));
  TRY(dmalloc(&h->d_fext, 3 * N));
  HIP_TRY(hipMemset(h->d_fext, 0, 3 * N * sizeof(double)));
  return 0;
}

extern "C" int tlfea_t10_create(int n_elem, int n_nodes, tlfea_t10_t* out) {
  if (!out || n_elem <= 0 || n_nodes <= 0) return fail("tlfea_t10_create: bad arguments");
  if (tlfea_device_count() <= 0) return fail("tlfea_t10_create: no HIP device visible (this engine has no CPU path)");
  auto* h = new tlfea_t10_s();
  h->E = n_elem;
  h->N = h->n_nodes = n_nodes;
  TRY(alloc_common(h));
  *out = h;
  return 0;
}

// GPU_ANCF3243_Data(int n_nodes, int n_elements) / GPU_ANCF3443_Data(int n_nodes, int n_elements) + Initialize()
// (ANCF3243Data.cuh:434-509, ANCF3443Data.cuh:445-520).  kind = 3243 | 3443.
extern "C" int tlfea_ancf_create(int kind, int n_nodes, int n_elements, tlfea_t10_t* out) {
  if (!out || n_elements <= 0 || n_nodes <= 0 || (kind != 3243 && kind != 3443))
    return fail("tlfea_ancf_create: bad arguments");
  if (tlfea_device_count() <= 0) return fail("tlfea_ancf_create: no HIP device visible (this engine has no CPU path)");
  auto* h = new tlfea_t10_s();
  h->kind = kind == 3243 ? kANCF3243 : kANCF3443;
  h->S = kind == 3243 ? 8 : 16;
  h->Q = kind == 3243 ? 12 : 48;
  h->nn = h->S / 4;
  h->E = n_elements;
  h->n_nodes = n_nodes;
  h->N = 4 * n_nodes;  // coefficient vectors r, r_u, r_v, r_w per node
  TRY(alloc_common(h));
  *out = h;
  return 0;
}

extern "C" int tlfea_t10_destroy(tlfea_t10_t h) {
  if (!h) return 0;
  void* ptrs[] = {h->d_conn, h->d_x, h->d_y, h->d_z, h->d_xt, h->d_yt, h->d_zt, h->d_qx, h->d_qy, h->d_qz,
                  h->d_gradN, h->d_gradN_t, h->d_detJ, h->d_F, h->d_P, h->d_Fdot, h->d_Pvis, h->d_fbuf, h->d_fint,
                  h->d_fext, h->d_cons, h->d_fixed, h->d_fixed_slot, h->d_off, h->d_cols, h->d_n2e_off, h->d_n2e,
                  h->d_n2e_pos, h->d_diagpos, h->d_mval, h->d_joff, h->d_jcol, h->d_jtoff, h->d_jtcol, h->d_jval,
                  h->d_jtval, h->d_rhs, h->d_emat, h->d_ob_node, h->d_ob_w, h->d_ob_f, h->d_ob_blk, h->d_ob_fk,
                  h->d_ob_res, h->d_st_pts, h->d_st_erec, h->d_st_contrib, h->d_st_nodal, h->d_st_part, h->d_st_tot,
                  h->d_st_vel, h->d_st_noff, h->d_st_nel, h->d_ao_cls, h->d_ao_touched, h->d_ao_sval, h->d_ao_w,
                  h->d_ao_cbuf, h->d_ao_blk, h->d_ao_fk, h->d_ao_fc, h->d_ao_pts, h->d_ld_fc, h->d_ld_tr, h->d_ld_f,
                  h->d_ld_lbuf, h->d_ld_tab, h->d_ld_qw, h->d_ld_pe, h->d_ld_cls, h->d_ld_mask, h->d_ld_fnodes, h->d_ld_foff,
                  h->d_ld_fslot, h->d_fld, h->d_sn_sens, h->d_sn_part, h->d_sn_out, h->d_sn_w, h->d_sn_u, h->d_sn_pe,
                  h->d_sn_rho, h->d_sn_idx, h->d_sn_boff, h->d_sn_blk, h->d_sh_rows, h->d_sh_out, h->d_rc_rec, h->d_rc_nodal, h->d_rc_err,
                  h->d_rc_part, h->d_rc_tot, h->d_rc_pn, h->d_rc_pe, h->d_rc_dn, h->d_rc_de, h->d_rc_pts};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (double* p : h->d_fld_V)
    if (p) (void)hipFree(p);
  delete h;
  return 0;
}

extern "C" int tlfea_t10_setup(tlfea_t10_t h, const double* qx, const double* qy, const double* qz, const double* qw,
                               const double* x, const double* y, const double* z, const int* conn) {
  if (!h) return fail("null handle");
  if (h->is_setup) return fail("GPU_FEAT10_Data is already set up.");
  if (h->kind != kT10) return fail("tlfea_t10_setup called on an ANCF handle");
  const size_t N = h->N, E = h->E;
  for (size_t k = 0; k < E * kNN; k++)
    if (conn[k] < 0 || conn[k] >= h->N) return fail("tlfea_t10_setup: connectivity index out of range");
  HIP_TRY(hipMemcpy(h->d_x, x, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_y, y, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_z, z, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_xt, x, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_yt, y, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_zt, z, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_conn, conn, E * kNN * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_qx, qx, kNQ * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_qy, qy, kNQ * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_qz, qz, kNQ * sizeof(double), hipMemcpyHostToDevice));
  for (int q = 0; q < kNQ; q++) {
    h->h_qw[q] = qw[q];
    h->h_q[0][q] = qx[q];
    h->h_q[1][q] = qy[q];
    h->h_q[2][q] = qz[q];
  }
  h->h_conn.assign(conn, conn + E * kNN);
  h->h_X0.resize(3 * N);
  std::copy(x, x + N, h->h_X0.begin());
  std::copy(y, y + N, h->h_X0.begin() + N);
  std::copy(z, z + N, h->h_X0.begin() + 2 * N);
  HIP_TRY(hipMemset(h->d_gradN, 0, E * kNQ * 30 * sizeof(double)));
  HIP_TRY(hipMemset(h->d_gradN_t, 0, (size_t)h->Epad * kNQ * 30 * sizeof(double)));
  HIP_TRY(hipMemset(h->d_detJ, 0, E * kNQ * sizeof(double)));
  HIP_TRY(hipMemset(h->d_fint, 0, 3 * N * sizeof(double)));
  HIP_TRY(hipMemset(h->d_fbuf, 0, E * 30 * sizeof(double)));
  h->mat = Material{kSVK, 0, 0, 0, 0, 0, 0, 0, 0};  // FEAT10Data.cuh:494-506
  h->is_setup = true;
  return 0;
}

#define NO_TABLE(h, what)                                                                                               \
  if ((h)->d_emat)                                                                                                    \
  return fail(std::string(what) + ": per-element materials are set (tlfea_t10_set_element_materials); clear them first " \
                                  "(tlfea_t10_clear_element_materials)")

extern "C" int tlfea_t10_set_density(tlfea_t10_t h, double rho0) {
  NEED_SETUP(h, "setting density.");
  NO_TABLE(h, "tlfea_t10_set_density");
  h->gen++;
  h->mat.rho0 = rho0;
  return 0;
}
extern "C" int tlfea_t10_set_damping(tlfea_t10_t h, double eta, double lamd) {
  NEED_SETUP(h, "setting damping.");
  NO_TABLE(h, "tlfea_t10_set_damping");
  h->gen++;
  h->mat.eta = eta;
  h->mat.lamd = lamd;
  return 0;
}
extern "C" int tlfea_t10_set_svk_select(tlfea_t10_t h) {
  NEED_SETUP(h, "setting material.");
  NO_TABLE(h, "tlfea_t10_set_svk_select");
  h->gen++;
  h->mat.model = kSVK;
  h->mat.mu10 = h->mat.mu01 = h->mat.kappa = 0.0;
  return 0;
}
extern "C" int tlfea_t10_set_svk(tlfea_t10_t h, double E, double nu) {
  NEED_SETUP(h, "setting material.");
  NO_TABLE(h, "tlfea_t10_set_svk");
  h->E_mod = E;
  h->nu = nu;
  h->mat.mu = E / (2 * (1 + nu));
  h->mat.lambda = (E * nu) / ((1 + nu) * (1 - 2 * nu));
  return tlfea_t10_set_svk_select(h);
}
extern "C" int tlfea_t10_set_mooney_rivlin(tlfea_t10_t h, double mu10, double mu01, double kappa) {
  NEED_SETUP(h, "setting material.");
  NO_TABLE(h, "tlfea_t10_set_mooney_rivlin");
  h->gen++;
  h->mat.model = kMooneyRivlin;
  h->mat.mu10 = mu10;
  h->mat.mu01 = mu01;
  h->mat.kappa = kappa;
  return 0;
}
// ---- per-element materials --------------------------------------------------------------------------------------------
// the device records of every element: the entry of its id, with the density its mass-matrix share was assembled with
static int upload_emat(tlfea_t10_t h) {
  const int E = h->E;
  std::vector<double> rec((size_t)E * kEmRec);
  for (int e = 0; e < E; e++) {
    std::copy_n(&h->h_table[(size_t)h->h_eid[e] * kEmRec], kEmRec, &rec[(size_t)e * kEmRec]);
    rec[(size_t)e * kEmRec + kEmRhoM] = h->h_rho_mass[e];
  }
  if (!h->d_emat) TRY(dmalloc(&h->d_emat, rec.size()));
  HIP_TRY(hipMemcpy(h->d_emat, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}
extern "C" int tlfea_t10_set_element_materials(tlfea_t10_t h, int model, int n_mat, const tlfea_material_entry* table,
                                               const int* elem_material, int n_elem) {
  if (h && h->kind != kT10) return fail("tlfea_t10_set_element_materials: T10 handles only (not an ANCF handle)");
  NEED_SETUP(h, "setting element materials.");
  if (model != kSVK && model != kMooneyRivlin)
    return fail("tlfea_t10_set_element_materials: unknown model " + std::to_string(model) + " (0 SVK, 1 Mooney-Rivlin)");
  if (n_mat < 1 || n_mat > kMaxMaterials)
    return fail("tlfea_t10_set_element_materials: n_mat must be in 1.." + std::to_string(kMaxMaterials) + ", got " +
                std::to_string(n_mat));
  if (!table || !elem_material) return fail("tlfea_t10_set_element_materials: null table or element ids");
  if (n_elem != h->E)
    return fail("tlfea_t10_set_element_materials: n_elem " + std::to_string(n_elem) + " != number of elements " +
                std::to_string(h->E));
  for (int e = 0; e < n_elem; e++)
    if (elem_material[e] < 0 || elem_material[e] >= n_mat)
      return fail("tlfea_t10_set_element_materials: element " + std::to_string(e) + " has material id " +
                  std::to_string(elem_material[e]) + " outside 0.." + std::to_string(n_mat - 1));
  std::vector<double> tab((size_t)n_mat * kEmRec);
  bool damp = false;
  for (int k = 0; k < n_mat; k++) {
    const tlfea_material_entry& t = table[k];
    if (model == kSVK && !(t.nu > -1.0 && t.nu < 0.5))
      return fail("tlfea_t10_set_element_materials: entry " + std::to_string(k) + ": nu must be in (-1, 0.5)");
    if (!(t.rho0 >= 0.0)) return fail("tlfea_t10_set_element_materials: entry " + std::to_string(k) + ": negative density");
    double* r = &tab[(size_t)k * kEmRec];
    // the same arithmetic as tlfea_t10_set_svk: a one-entry table reproduces the uniform path
    r[kEmMu] = model == kSVK ? t.E / (2 * (1 + t.nu)) : 0.0;
    r[kEmLambda] = model == kSVK ? (t.E * t.nu) / ((1 + t.nu) * (1 - 2 * t.nu)) : 0.0;
    r[kEmEta] = t.eta;
    r[kEmLamd] = t.lamd;
    r[kEmMu10] = model == kMooneyRivlin ? t.mu10 : 0.0;
    r[kEmMu01] = model == kMooneyRivlin ? t.mu01 : 0.0;
    r[kEmKappa] = model == kMooneyRivlin ? t.kappa : 0.0;
    r[kEmRhoM] = t.rho0;
    damp = damp || t.eta != 0.0 || t.lamd != 0.0;
  }
  // launches in flight on a solver's stream may still read the old records
  HIP_TRY(hipDeviceSynchronize());
  if (!h->d_emat) {
    h->mat_saved = h->mat;
    // the mass matrix assembled so far (uniform density) stays until the next CalcMassMatrix
    h->h_rho_mass.assign(h->E, h->mass_rho0 > 0.0 ? h->mass_rho0 : 0.0);
  }
  h->h_table.swap(tab);
  h->h_eid.assign(elem_material, elem_material + n_elem);
  h->n_mat = n_mat;
  h->emat_damp = damp;
  h->mat.model = model;
  TRY(upload_emat(h));
  h->gen++;
  return 0;
}
extern "C" int tlfea_t10_clear_element_materials(tlfea_t10_t h) {
  NEED_SETUP(h, "clearing element materials.");
  if (!h->d_emat) return 0;
  HIP_TRY(hipDeviceSynchronize());
  (void)hipFree(h->d_emat);
  h->d_emat = nullptr;
  h->mat = h->mat_saved;
  if (h->mass_pe) {
    // a mass matrix of per-element densities has no uniform density: it is dropped until the next CalcMassMatrix
    if (h->d_mval && h->nnz_coef > 0) HIP_TRY(hipMemset(h->d_mval, 0, (size_t)h->nnz_coef * sizeof(double)));
    h->mass_rho0 = -1.0;
    h->mass_pe = false;
  }
  h->n_mat = 0;
  h->emat_damp = false;
  h->h_table.clear();
  h->h_eid.clear();
  h->h_rho_mass.clear();
  h->gen++;
  return 0;
}
extern "C" int tlfea_t10_get_element_materials(tlfea_t10_t h, int* n_mat, int* elem_material) {
  if (!h) return fail("null handle");
  if (n_mat) *n_mat = h->n_mat;
  if (elem_material && h->d_emat) std::copy(h->h_eid.begin(), h->h_eid.end(), elem_material);
  return 0;
}

extern "C" int tlfea_t10_set_external_force(tlfea_t10_t h, const double* f, int n) {
  if (!h) return fail("null handle");
  if (n != 3 * h->N) return fail("External force vector size mismatch.");
  HIP_TRY(hipMemcpy(h->d_fext, f, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

static int upload_fixed(tlfea_t10_t h, const int* nodes, int n_fixed) {
  for (int k = 0; k < n_fixed; k++)
    if (nodes[k] < 0 || nodes[k] >= h->N) return fail("fixed node index out of range");
  // a solver may still have launches in flight that read the old buffers (its own stream): drain before freeing
  HIP_TRY(hipDeviceSynchronize());
  h->gen++;
  if (h->d_cons) (void)hipFree(h->d_cons);
  if (h->d_fixed) (void)hipFree(h->d_fixed);
  if (h->d_fixed_slot) (void)hipFree(h->d_fixed_slot);
  h->n_fixed = n_fixed;
  h->n_constraint = 3 * n_fixed;
  h->h_fixed.assign(nodes, nodes + n_fixed);
  TRY(dmalloc(&h->d_cons, (size_t)h->n_constraint));
  TRY(dmalloc(&h->d_fixed, (size_t)n_fixed));
  TRY(dmalloc(&h->d_fixed_slot, (size_t)h->N));
  HIP_TRY(hipMemset(h->d_cons, 0, std::max(1, h->n_constraint) * sizeof(double)));
  std::vector<int> slot(h->N, -1);
  for (int k = 0; k < n_fixed; k++) slot[nodes[k]] = k;  // a node listed twice keeps its last slot
  if (n_fixed) HIP_TRY(hipMemcpy(h->d_fixed, nodes, (size_t)n_fixed * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_fixed_slot, slot.data(), (size_t)h->N * sizeof(int), hipMemcpyHostToDevice));
  h->is_constraints_setup = true;
  h->cons_mode = 1;
  h->is_j_csr_setup = h->is_cj_csr_setup = false;
  return 0;
}

extern "C" int tlfea_t10_set_nodal_fixed(tlfea_t10_t h, const int* nodes, int n_fixed) {
  if (!h) return fail("null handle");
  if (h->is_constraints_setup) return fail("GPU_FEAT10_Data CONSTRAINT is already set up.");
  return upload_fixed(h, nodes, n_fixed);
}
extern "C" int tlfea_t10_update_nodal_fixed(tlfea_t10_t h, const int* nodes, int n_fixed) {
  if (!h) return fail("null handle");
  return upload_fixed(h, nodes, n_fixed);
}
// SetLinearConstraintsCSR (ANCF3243Data.cuh:810-940, ANCF3443Data.cuh same): c = J x - rhs over the flattened DOF
// vector (3*coef + component).  Uploads J and builds J^T (counting sort by column: entries of a DOF row stay in
// ascending constraint id, as the reference builds it).
extern "C" int tlfea_t10_set_linear_constraints_csr(tlfea_t10_t h, int n_rows, const int* offsets, const int* columns,
                                                    const double* values, const double* rhs) {
  if (!h) return fail("null handle");
  if (h->is_constraints_setup) return fail("CONSTRAINT is already set up.");
  if (n_rows < 0 || !offsets || offsets[0] != 0) return fail("SetLinearConstraintsCSR: invalid offsets.");
  const int nnz = offsets[n_rows];
  for (int r = 0; r < n_rows; r++)
    if (offsets[r + 1] < offsets[r]) return fail("SetLinearConstraintsCSR: invalid offsets.");
  const int n_dofs = 3 * h->N;
  for (int k = 0; k < nnz; k++)
    if (columns[k] < 0 || columns[k] >= n_dofs) return fail("SetLinearConstraintsCSR: column out of range.");
  // the coefficient adjacency (mass / Hessian pattern) must include the pairs a constraint row couples
  if (h->is_csr_setup)
    return fail("SetLinearConstraintsCSR must precede BuildMassCSRPattern / CalcMassMatrix (the Hessian pattern "
                "includes the coefficient pairs coupled by constraint rows)");
  h->n_fixed = 0;
  h->n_constraint = n_rows;
  h->cons_mode = 2;
  h->h_joff.assign(offsets, offsets + n_rows + 1);
  h->h_jcol.assign(columns, columns + nnz);
  h->h_jval.assign(values, values + nnz);
  h->h_rhs.assign(rhs, rhs + n_rows);
  h->h_jtoff.assign((size_t)n_dofs + 1, 0);
  h->h_jtcol.assign((size_t)nnz, 0);
  h->h_jtval.assign((size_t)nnz, 0.0);
  for (int k = 0; k < nnz; k++) h->h_jtoff[(size_t)columns[k] + 1]++;
  for (int i = 0; i < n_dofs; i++) h->h_jtoff[(size_t)i + 1] += h->h_jtoff[i];
  {
    std::vector<int> cur(h->h_jtoff.begin(), h->h_jtoff.end() - 1);
    for (int r = 0; r < n_rows; r++)
      for (int k = offsets[r]; k < offsets[r + 1]; k++) {
        const int o = cur[columns[k]]++;
        h->h_jtcol[o] = r;
        h->h_jtval[o] = values[k];
      }
  }
  TRY(dmalloc(&h->d_cons, (size_t)std::max(1, n_rows)));
  HIP_TRY(hipMemset(h->d_cons, 0, (size_t)std::max(1, n_rows) * sizeof(double)));
  TRY(dmalloc(&h->d_rhs, (size_t)std::max(1, n_rows)));
  TRY(dmalloc(&h->d_joff, (size_t)n_rows + 1));
  TRY(dmalloc(&h->d_jcol, (size_t)std::max(1, nnz)));
  TRY(dmalloc(&h->d_jval, (size_t)std::max(1, nnz)));
  TRY(dmalloc(&h->d_jtoff, (size_t)n_dofs + 1));
  TRY(dmalloc(&h->d_jtcol, (size_t)std::max(1, nnz)));
  TRY(dmalloc(&h->d_jtval, (size_t)std::max(1, nnz)));
  if (n_rows) HIP_TRY(hipMemcpy(h->d_rhs, rhs, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_joff, offsets, ((size_t)n_rows + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_jtoff, h->h_jtoff.data(), ((size_t)n_dofs + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (nnz) {
    HIP_TRY(hipMemcpy(h->d_jcol, columns, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_jval, values, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_jtcol, h->h_jtcol.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_jtval, h->h_jtval.data(), (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
  }
  h->is_j_csr_setup = h->is_cj_csr_setup = true;
  h->is_constraints_setup = true;
  return 0;
}
// GetConstraintMode: 0 none, 1 kConstraintFixedCoefficients, 2 kConstraintLinearCSR
extern "C" int tlfea_t10_update_linear_constraint_rhs(tlfea_t10_t h, const double* rhs, int n) {
  if (!h->is_constraints_setup || h->n_constraint == 0) return fail("UpdateLinearConstraintRHS: constraints not set up.");
  if (h->cons_mode != 2) return fail("UpdateLinearConstraintRHS: constraint mode is not CSR.");
  if (n != h->n_constraint) return fail("UpdateLinearConstraintRHS: size mismatch.");
  h->h_rhs.assign(rhs, rhs + n);
  HIP_TRY(hipMemcpy(h->d_rhs, rhs, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}
extern "C" int tlfea_t10_get_constraint_mode(tlfea_t10_t h) { return h ? h->cons_mode : -1; }
extern "C" int tlfea_t10_constraint_jac_nnz(tlfea_t10_t h) {
  if (!h || !h->is_constraints_setup) return 0;
  return h->cons_mode == 2 ? (int)h->h_jcol.size() : h->n_constraint;
}

extern "C" int tlfea_t10_update_positions(tlfea_t10_t h, const double* x, const double* y, const double* z, int n) {
  if (!h || n != h->N) return fail("Position vector size mismatch.");
  HIP_TRY(hipMemcpy(h->d_x, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_y, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_z, z, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}
extern "C" int tlfea_t10_update_constraint_targets(tlfea_t10_t h, const double* x, const double* y, const double* z,
                                                   int n) {
  if (!h || n != h->N) return fail("Position vector size mismatch.");
  HIP_TRY(hipMemcpy(h->d_xt, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_yt, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_zt, z, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

extern "C" int tlfea_ancf_calc_dsdu_pre(tlfea_t10_t h);
extern "C" int tlfea_t10_calc_dndu_pre(tlfea_t10_t h) {
  NEED_SETUP(h, "CalcDnDuPre.");
  if (h->kind != kT10) return tlfea_ancf_calc_dsdu_pre(h);
  launch_dndu_pre(h->stream, h->E, h->Epad, h->d_conn, h->d_x, h->d_y, h->d_z, h->d_qx, h->d_qy, h->d_qz, h->d_gradN,
                  h->d_gradN_t, h->d_detJ);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  h->have_dndu = true;
  h->geom_gen++;
  return 0;
}

// Node adjacency (== mass CSR pattern, FEAT10Data.cu:372-440: sorted unique (row,col) pairs) built on
// the host from the node->element incidence, together with the gather-assembly scatter map.
extern "C" int tlfea_t10_build_mass_csr_pattern(tlfea_t10_t h) {
  NEED_SETUP(h, "BuildMassCSRPattern.");
  if (h->is_csr_setup) return 0;
  const int E = h->E, N = h->N, S = h->S;
  const int* conn = h->h_conn.data();
  std::vector<int>& n2e_off = h->h_n2e_off;
  std::vector<int>& n2e = h->h_n2e;
  n2e_off.assign(N + 1, 0);
  for (int a = 0; a < S; a++)
    for (int e = 0; e < E; e++) n2e_off[conn[(size_t)a * E + e] + 1]++;
  for (int i = 0; i < N; i++) n2e_off[i + 1] += n2e_off[i];
  n2e.assign((size_t)E * S, 0);
  {
    std::vector<int> cur(n2e_off.begin(), n2e_off.end() - 1);
    for (int e = 0; e < E; e++)  // ascending e per node -> fixed summation order
      for (int a = 0; a < S; a++) n2e[cur[conn[(size_t)a * E + e]]++] = e * S + a;
  }
  // coefficient pairs coupled by a general linear constraint row are adjacent too (SyncedNewton.cu:597-624):
  // J^T J fills their 3x3 blocks.  cadj = per-coefficient list of such partners (CSR, unsorted, with duplicates).
  std::vector<int> cadj_off(N + 1, 0), cadj;
  if (h->cons_mode == 2 && h->n_constraint > 0) {
    std::vector<int> row_coefs;
    for (int pass = 0; pass < 2; pass++) {
      std::vector<int> cur(cadj_off.begin(), cadj_off.end() - 1);
      for (int r = 0; r < h->n_constraint; r++) {
        row_coefs.clear();
        for (int k = h->h_joff[r]; k < h->h_joff[r + 1]; k++) row_coefs.push_back(h->h_jcol[k] / 3);
        std::sort(row_coefs.begin(), row_coefs.end());
        row_coefs.erase(std::unique(row_coefs.begin(), row_coefs.end()), row_coefs.end());
        for (int a : row_coefs)
          for (int b : row_coefs) {
            if (pass == 0) cadj_off[a + 1]++;
            else cadj[cur[a]++] = b;
          }
      }
      if (pass == 0) {
        for (int i = 0; i < N; i++) cadj_off[i + 1] += cadj_off[i];
        cadj.assign((size_t)cadj_off[N], 0);
      }
    }
  }
  std::vector<int> deg(N, 0), deg_elem(N, 0);
  h->h_off.assign(N + 1, 0);
  std::vector<size_t> tmp_off(N + 1, 0);
  for (int i = 0; i < N; i++)
    tmp_off[i + 1] = tmp_off[i] + (size_t)(n2e_off[i + 1] - n2e_off[i]) * S + (size_t)(cadj_off[i + 1] - cadj_off[i]) + 1;
  std::vector<int> tmp_cols(tmp_off[N]), tmp_elem(tmp_off[N]);  // upper bounds, compacted below
#pragma omp parallel for schedule(dynamic, 1024)
  for (int i = 0; i < N; i++) {
    int* c = tmp_cols.data() + tmp_off[i];
    int* ce = tmp_elem.data() + tmp_off[i];
    int n = 0;
    for (int k = n2e_off[i]; k < n2e_off[i + 1]; k++) {
      const int e = n2e[k] / S;
      for (int a = 0; a < S; a++) c[n++] = conn[(size_t)a * E + e];
    }
    std::sort(c, c + n);
    n = (int)(std::unique(c, c + n) - c);
    std::copy(c, c + n, ce);  // the element-only adjacency == mass pattern
    deg_elem[i] = n;
    if (cadj_off[i + 1] > cadj_off[i]) {
      for (int k = cadj_off[i]; k < cadj_off[i + 1]; k++) c[n++] = cadj[k];
      c[n++] = i;  // the reference seeds every row with its diagonal (SyncedNewton.cu:577-580)
      std::sort(c, c + n);
      n = (int)(std::unique(c, c + n) - c);
    }
    deg[i] = n;
  }
  long long nnz = 0;
  int maxdeg = 0;
  for (int i = 0; i < N; i++) {
    h->h_off[i] = (int)nnz;
    nnz += deg[i];
    maxdeg = std::max(maxdeg, deg[i]);
  }
  if (nnz * 9 >= (1LL << 31)) return fail("Hessian nnz exceeds int32 CSR offsets (SyncedNewton.cuh:385-388)");
  h->h_off[N] = (int)nnz;
  h->nnz_coef = (int)nnz;
  h->maxdeg = maxdeg;
  h->h_cols.resize((size_t)nnz);
  h->h_extra.assign((size_t)nnz, 0);
  std::vector<int> pos((size_t)E * S * S), diagpos(N, 0);
  long long n_extra = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : n_extra)
  for (int i = 0; i < N; i++) {
    const int* c = tmp_cols.data() + tmp_off[i];
    const int* ce = tmp_elem.data() + tmp_off[i];
    int* dst = h->h_cols.data() + h->h_off[i];
    std::copy(c, c + deg[i], dst);
    if (deg[i] != deg_elem[i])
      for (int k = 0; k < deg[i]; k++)
        if (!std::binary_search(ce, ce + deg_elem[i], dst[k])) {
          h->h_extra[(size_t)h->h_off[i] + k] = 1;
          n_extra++;
        }
    diagpos[i] = (int)(std::lower_bound(dst, dst + deg[i], i) - dst);
    for (int k = n2e_off[i]; k < n2e_off[i + 1]; k++) {
      const int e = n2e[k] / S;
      for (int a = 0; a < S; a++)
        pos[(size_t)k * S + a] = (int)(std::lower_bound(dst, dst + deg[i], conn[(size_t)a * E + e]) - dst);
    }
  }
  h->nnz_mass = (int)(nnz - n_extra);
  TRY(dmalloc(&h->d_off, (size_t)N + 1));
  TRY(dmalloc(&h->d_cols, (size_t)nnz));
  TRY(dmalloc(&h->d_n2e_off, (size_t)N + 1));
  TRY(dmalloc(&h->d_n2e, (size_t)E * S));
  TRY(dmalloc(&h->d_n2e_pos, (size_t)E * S * S));
  TRY(dmalloc(&h->d_diagpos, (size_t)N));
  TRY(dmalloc(&h->d_mval, (size_t)nnz));
  HIP_TRY(hipMemcpy(h->d_off, h->h_off.data(), ((size_t)N + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_cols, h->h_cols.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_n2e_off, n2e_off.data(), ((size_t)N + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_n2e, n2e.data(), (size_t)E * S * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_n2e_pos, pos.data(), (size_t)E * S * S * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_diagpos, diagpos.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(h->d_mval, 0, (size_t)nnz * sizeof(double)));
  h->is_csr_setup = true;
  return 0;
}

static int ancf_mass_host(tlfea_t10_t h);
extern "C" int tlfea_t10_calc_mass_matrix(tlfea_t10_t h) {
  NEED_SETUP(h, "CalcMassMatrix.");
  if (!h->is_csr_setup) TRY(tlfea_t10_build_mass_csr_pattern(h));
  if (h->kind != kT10) return ancf_mass_host(h);
  if (h->d_emat) {
    // per-element densities: the snapshot of the table's densities goes into the records' kEmRhoM slot first
    HIP_TRY(hipDeviceSynchronize());
    for (int e = 0; e < h->E; e++) h->h_rho_mass[e] = h->h_table[(size_t)h->h_eid[e] * kEmRec + kEmRhoM];
    TRY(upload_emat(h));
    h->gen++;
  }
  launch_mass_values(h->stream, h->view(), h->inc(), h->d_qx, h->d_qy, h->d_qz, h->mat.rho0, h->d_mval, h->d_emat);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  // per-element: 1 flags an assembled mass (the solvers scale by 1/h and take each element's density from its record)
  h->mass_rho0 = h->d_emat ? 1.0 : h->mat.rho0;
  h->mass_pe = h->d_emat != nullptr;
  h->ld_const_dirty = true;  // the body force follows the mass matrix
  return 0;
}

// A new reference geometry for the same connectivity: grad N, det J and the mass values again from X, with
// everything derived from the reference coordinates on the host marked stale.  The current positions, velocities,
// multipliers and targets are the caller's.  An inverted element refuses the call before anything is touched.
extern "C" int tlfea_t10_set_reference_positions(tlfea_t10_t h, const double* x, const double* y, const double* z, int n) {
  const char* what = "tlfea_t10_set_reference_positions";
  if (h && h->kind != kT10) return fail(std::string(what) + ": T10 handles only (not an ANCF handle)");
  NEED_SETUP(h, "setting reference positions.");
  if (!x || !y || !z) return fail(std::string(what) + ": null coordinates");
  if (n != h->N) return fail(std::string(what) + ": " + std::to_string(n) + " nodes given, the object has " + std::to_string(h->N));
  const int E = h->E, N = h->N;
  // det J at every point of the rule, as dndu_pre_kernel forms it
  const int edges[6][2] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {1, 3}, {2, 3}};
  const double dL[4][3] = {{-1, -1, -1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  double dN[kNQ][kNN][3];
  for (int q = 0; q < kNQ; q++) {
    const double L[4] = {1.0 - h->h_q[0][q] - h->h_q[1][q] - h->h_q[2][q], h->h_q[0][q], h->h_q[1][q], h->h_q[2][q]};
    for (int i = 0; i < 4; i++)
      for (int d = 0; d < 3; d++) dN[q][i][d] = (4.0 * L[i] - 1.0) * dL[i][d];
    for (int k = 0; k < 6; k++)
      for (int d = 0; d < 3; d++)
        dN[q][k + 4][d] = 4.0 * (L[edges[k][0]] * dL[edges[k][1]][d] + L[edges[k][1]] * dL[edges[k][0]][d]);
  }
  int bad = E;
#pragma omp parallel for schedule(static) reduction(min : bad)
  for (int e = 0; e < E; e++)
    for (int q = 0; q < kNQ; q++) {
      double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int a = 0; a < kNN; a++) {
        const int g = h->h_conn[(size_t)a * E + e];
        const double X[3] = {x[g], y[g], z[g]};
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) J[i][j] += X[i] * dN[q][a][j];
      }
      const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                         J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
      if (!(det > 0.0)) bad = std::min(bad, e);
    }
  if (bad < E)
    return fail(std::string(what) + ": element " + std::to_string(bad) + " is inverted (det J <= 0 at a quadrature point); the "
                "reference geometry is unchanged");
  HIP_TRY(hipDeviceSynchronize());  // launches in flight on a solver's stream may still read the old geometry
  double* d_X = nullptr;
  TRY(dmalloc(&d_X, 3 * (size_t)N));
  int rc = 0;
  const double* src[3] = {x, y, z};
  for (int c = 0; c < 3 && !rc; c++)
    if (hipMemcpy(d_X + (size_t)c * N, src[c], (size_t)N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(std::string(what) + ": upload failed");
  if (!rc) {
    launch_dndu_pre(h->stream, E, h->Epad, h->d_conn, d_X, d_X + N, d_X + 2 * (size_t)N, h->d_qx, h->d_qy, h->d_qz, h->d_gradN,
                    h->d_gradN_t, h->d_detJ);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = fail(std::string(what) + ": grad N launch failed");
  }
  (void)hipFree(d_X);
  if (rc) return rc;
  h->have_dndu = true;
  h->geom_gen++;
  std::copy(x, x + N, h->h_X0.begin());
  std::copy(y, y + N, h->h_X0.begin() + N);
  std::copy(z, z + N, h->h_X0.begin() + 2 * (size_t)N);
  if (h->mass_rho0 >= 0.0 && h->d_mval) {
    // the same pattern and the densities the matrix was assembled with (under a table: slot kEmRhoM of the records)
    launch_mass_values(h->stream, h->view(), h->inc(), h->d_qx, h->d_qy, h->d_qz, h->mass_rho0, h->d_mval, h->d_emat);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  h->ld_const_dirty = true;  // M a and the traction vector follow the reference geometry
  if (h->bf_built) {
    h->bf_built = false;  // outward orientation is decided from the reference coordinates
    boundary_faces_build(h);
    if (h->ld_n_trac > 0) TRY(t10_loads_build_traction(h));
  }
  TRY(t10_surface_refresh(h));
  return 0;
}

// Setup(length,width,height per element, mass rule, force rule, x12,y12,z12, connectivity)
// (ANCF3243Data.cuh:511-651 and its scalar overload :653-670; ANCF3443Data.cuh:522-670).
// rules: gauss/weight arrays in the order xi_m, eta_m, zeta_m (mass) and xi, eta, zeta (force);
// conn_nodes: E x nn node ids, row-major [e][k] (set conn_is_colmajor for an Eigen-style E x nn matrix).
extern "C" int tlfea_ancf_setup(tlfea_t10_t h, const double* L, const double* W, const double* H,
                                const double* gxm, const double* gym, const double* gzm, const double* wxm,
                                const double* wym, const double* wzm, const int* nqm, const double* gx,
                                const double* gy, const double* gz, const double* wx, const double* wy,
                                const double* wz, const int* nq, const double* x12, const double* y12,
                                const double* z12, const int* conn_nodes, int conn_is_colmajor) {
  if (!h || h->kind == kT10) return fail("tlfea_ancf_setup: not an ANCF handle");
  if (h->is_setup) return fail("GPU_ANCF data is already set up.");
  const int E = h->E, S = h->S, nn = h->nn;
  if (nq[0] * nq[1] * nq[2] != h->Q) return fail("tlfea_ancf_setup: force rule does not match the element type");
  const size_t N = h->N;
  std::vector<int> conn((size_t)S * E);
  for (int e = 0; e < E; e++)
    for (int k = 0; k < nn; k++) {
      const int node = conn_is_colmajor ? conn_nodes[(size_t)k * E + e] : conn_nodes[(size_t)e * nn + k];
      if (node < 0 || node >= h->n_nodes) return fail("tlfea_ancf_setup: connectivity index out of range");
      for (int d = 0; d < 4; d++) conn[(size_t)(4 * k + d) * E + e] = 4 * node + d;  // coef = 4*node + slot
    }
  h->h_conn = conn;
  h->Lv.assign(L, L + E); h->Wv.assign(W, W + E); h->Hv.assign(H, H + E);
  const double* fr[6] = {gx, gy, gz, wx, wy, wz};
  const double* mr[6] = {gxm, gym, gzm, wxm, wym, wzm};
  for (int k = 0; k < 6; k++) {
    h->fr[k].assign(fr[k], fr[k] + nq[k % 3]);
    h->mr[k].assign(mr[k], mr[k] + nqm[k % 3]);
  }
  for (int q = 0; q < h->Q; q++)  // qp = (ixi*n_eta + ieta)*n_zeta + izeta  (ANCF3243DataFunc.cuh:432-434)
    h->h_qw[q] = wx[q / (nq[1] * nq[2])] * wy[(q / nq[2]) % nq[1]] * wz[q % nq[2]];
  h->Binv.resize((size_t)E * S * S);
  for (int e = 0; e < E; e++)
    if (!ancf::B_inv(S, L[e], W[e], &h->Binv[(size_t)e * S * S])) return fail("tlfea_ancf_setup: singular B matrix");
  HIP_TRY(hipMemcpy(h->d_x, x12, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_y, y12, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_z, z12, N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_xt, x12, N * sizeof(double), hipMemcpyHostToDevice));  // x12_jac: reference geometry
  HIP_TRY(hipMemcpy(h->d_yt, y12, N * sizeof(double), hipMemcpyHostToDevice));  // AND constraint targets
  HIP_TRY(hipMemcpy(h->d_zt, z12, N * sizeof(double), hipMemcpyHostToDevice));  // (ANCF3243Data.cuh:576-587)
  HIP_TRY(hipMemcpy(h->d_conn, conn.data(), conn.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(h->d_fint, 0, 3 * N * sizeof(double)));
  HIP_TRY(hipMemset(h->d_fbuf, 0, (size_t)E * 3 * S * sizeof(double)));
  h->mat = Material{kSVK, 0, 0, 0, 0, 0, 0, 0, 0};
  h->is_setup = true;
  return 0;
}

// CalcDsDuPre (ANCF3243Data.cu:102-198 / ANCF3443Data.cu:96-182): reference gradients and det J from the
// x12_jac coefficients.  One-time set-up, done on the host and uploaded in both device layouts.
extern "C" int tlfea_ancf_calc_dsdu_pre(tlfea_t10_t h) {
  NEED_SETUP(h, "CalcDsDuPre.");
  if (h->kind == kT10) return fail("tlfea_ancf_calc_dsdu_pre: not an ANCF handle");
  const int E = h->E, S = h->S, Q = h->Q, Epad = h->Epad;
  const size_t N = h->N;
  std::vector<double> xj(N), yj(N), zj(N);
  HIP_TRY(hipMemcpy(xj.data(), h->d_xt, N * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(yj.data(), h->d_yt, N * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(zj.data(), h->d_zt, N * sizeof(double), hipMemcpyDeviceToHost));
  const int n1 = (int)h->fr[1].size(), n2 = (int)h->fr[2].size();
  std::vector<double> gN((size_t)E * Q * 3 * S), gNt((size_t)Epad * Q * 3 * S, 0.0), dJ((size_t)E * Q);
#pragma omp parallel for schedule(static)
  for (int e = 0; e < E; e++) {
    int coefs[kMaxS];
    for (int a = 0; a < S; a++) coefs[a] = h->h_conn[(size_t)a * E + e];
    for (int q = 0; q < Q; q++) {
      const int ix = q / (n1 * n2), ie = (q / n2) % n1, iz = q % n2;
      double ds[3][16], J[3][3], JT[3][3];
      ancf::ds_dxi(S, &h->Binv[(size_t)e * S * S], h->Lv[e], h->Wv[e], h->Hv[e], h->fr[0][ix], h->fr[1][ie], h->fr[2][iz], ds);
      dJ[(size_t)e * Q + q] = ancf::jacobian(S, coefs, xj.data(), yj.data(), zj.data(), ds, J);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) JT[i][j] = J[j][i];
      for (int a = 0; a < S; a++) {
        const double rhs[3] = {ds[0][a], ds[1][a], ds[2][a]};
        double g[3];
        ancf::solve3(JT, rhs, g);
        for (int d = 0; d < 3; d++) {
          gN[((size_t)e * Q + q) * 3 * S + (size_t)d * S + a] = g[d];
          gNt[((size_t)(q * 3 + d) * S + a) * Epad + e] = g[d];
        }
      }
    }
  }
  HIP_TRY(hipMemcpy(h->d_gradN, gN.data(), gN.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_gradN_t, gNt.data(), gNt.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_detJ, dJ.data(), dJ.size() * sizeof(double), hipMemcpyHostToDevice));
  h->have_dndu = true;
  // the sample-point weights of the obstacles (DESIGN 3e') belong to the reference this call has just used
  h->h_ao_w.clear();
  if (h->d_ao_w) {
    TRY(ancf_points_build(h));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->d_ao_w, h->h_ao_w.data(), h->h_ao_w.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  TRY(loads_build_traction(h));  // the traction vector is made of the same weights
  return 0;
}

// mass_matrix_qp_kernel of the ANCF types (ANCF3243Data.cu:200-288, ANCF3443Data.cu:184-254): mass rule,
// s = B_inv b, det J of the reference map; one-time set-up on the host, summed in element order.
static int ancf_mass_host(tlfea_t10_t h) {
  const int E = h->E, S = h->S;
  const size_t N = h->N;
  std::vector<double> xj(N), yj(N), zj(N), mval((size_t)h->nnz_coef, 0.0);
  HIP_TRY(hipMemcpy(xj.data(), h->d_xt, N * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(yj.data(), h->d_yt, N * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(zj.data(), h->d_zt, N * sizeof(double), hipMemcpyDeviceToHost));
  const int m0 = (int)h->mr[0].size(), m1 = (int)h->mr[1].size(), m2 = (int)h->mr[2].size();
  const ancf::Basis B = ancf::basis(S);
  // element-local S x S masses in parallel, then a row-owner gather in ascending element order (deterministic)
  std::vector<double> Me((size_t)E * S * S, 0.0);
#pragma omp parallel for schedule(static)
  for (int e = 0; e < E; e++) {
    int coefs[kMaxS];
    for (int a = 0; a < S; a++) coefs[a] = h->h_conn[(size_t)a * E + e];
    const double* Bi = &h->Binv[(size_t)e * S * S];
    double* M = &Me[(size_t)e * S * S];
    for (int q = 0; q < m0 * m1 * m2; q++) {
      const int ix = q / (m1 * m2), ie = (q / m2) % m1, iz = q % m2;
      const double wgt = h->mr[3][ix] * h->mr[4][ie] * h->mr[5][iz];
      double b[16], sv[16], ds[3][16], J[3][3];
      ancf::eval(B, h->Lv[e] * h->mr[0][ix] / 2, h->Wv[e] * h->mr[1][ie] / 2, h->Hv[e] * h->mr[2][iz] / 2, 0, b);
      for (int i = 0; i < S; i++) {
        double a = 0.0;
        for (int j = 0; j < S; j++) a += Bi[(size_t)j * S + i] * b[j];
        sv[i] = a;
      }
      ancf::ds_dxi(S, Bi, h->Lv[e], h->Wv[e], h->Hv[e], h->mr[0][ix], h->mr[1][ie], h->mr[2][iz], ds);
      const double detJ = ancf::jacobian(S, coefs, xj.data(), yj.data(), zj.data(), ds, J);
      for (int i = 0; i < S; i++)
        for (int j = 0; j < S; j++) M[i * S + j] += h->mat.rho0 * sv[i] * sv[j] * wgt * detJ;
    }
  }
#pragma omp parallel for schedule(static)
  for (int i = 0; i < (int)N; i++) {
    const int* row = h->h_cols.data() + h->h_off[i];
    const int deg = h->h_off[i + 1] - h->h_off[i];
    for (int k = h->h_n2e_off[i]; k < h->h_n2e_off[i + 1]; k++) {
      const int e = h->h_n2e[k] / S, il = h->h_n2e[k] % S;
      for (int j = 0; j < S; j++) {
        const int c = h->h_conn[(size_t)j * E + e];
        mval[h->h_off[i] + (int)(std::lower_bound(row, row + deg, c) - row)] += Me[((size_t)e * S + il) * S + j];
      }
    }
  }
  HIP_TRY(hipMemcpy(h->d_mval, mval.data(), mval.size() * sizeof(double), hipMemcpyHostToDevice));
  h->ancf_mass = true;
  h->ancf_mass_rho0 = h->mat.rho0;
  h->ld_const_dirty = true;  // the body force follows the mass matrix
  return 0;
}

extern "C" int tlfea_t10_calc_constraint_data(tlfea_t10_t h) {
  if (!h || !h->is_constraints_setup) return fail("constraint is not set up");
  if (h->n_constraint == 0) return 0;
  if (h->cons_mode == 2)
    launch_lin_constraint(h->stream, h->n_constraint, h->d_joff, h->d_jcol, h->d_jval, h->d_rhs, h->d_x, h->d_y, h->d_z,
                          h->d_cons);
  else
    launch_constraint(h->stream, h->n_fixed, h->d_fixed, h->d_x, h->d_y, h->d_z, h->d_xt, h->d_yt, h->d_zt, h->d_cons);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}
// J has one 1.0 per row (FEAT10Data.cu:443-459); J and J^T are implicit in fixed_nodes / fixed_slot on
// the device, the CSR forms are materialised only by the retrieve calls.
extern "C" int tlfea_t10_convert_to_csr_constraint_jac(tlfea_t10_t h) {
  if (!h) return fail("null handle");
  if (!h->is_constraints_setup || h->n_constraint == 0) return 0;
  h->is_j_csr_setup = true;
  return 0;
}
extern "C" int tlfea_t10_convert_to_csr_constraint_jact(tlfea_t10_t h) {
  if (!h) return fail("null handle");
  if (!h->is_constraints_setup || h->n_constraint == 0) return 0;
  h->is_cj_csr_setup = true;
  return 0;
}

static int ensure_fp_buffers(tlfea_t10_t h) {
  if (h->d_F) return 0;
  const size_t n = (size_t)h->E * h->Q * 9;
  TRY(dmalloc(&h->d_F, n)); TRY(dmalloc(&h->d_P, n)); TRY(dmalloc(&h->d_Fdot, n)); TRY(dmalloc(&h->d_Pvis, n));
  return 0;
}

extern "C" int tlfea_t10_calc_p(tlfea_t10_t h) {
  NEED_SETUP(h, "CalcP.");
  TRY(ensure_fp_buffers(h));
  // standalone CalcP passes a null v_guess: no viscous part (FEAT10Data.cu:302-304)
  launch_residual(h->stream, h->view(), h->mat, nullptr, h->d_fbuf, h->d_F, h->d_P, h->d_Fdot, h->d_Pvis, nullptr, nullptr, 0.0,
                  0x43210, h->d_emat);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  h->fbuf_valid = true;
  return 0;
}
extern "C" int tlfea_t10_calc_internal_force(tlfea_t10_t h) {
  NEED_SETUP(h, "CalcInternalForce.");
  if (!h->is_csr_setup) TRY(tlfea_t10_build_mass_csr_pattern(h));
  // d_fbuf holds the per-element force rows of the last residual evaluation (CalcP or the solver); a solver evaluation
  // on the interleaved-row path has written f_int itself (same P: the reference shares d_P between the two)
  if (h->fbuf_valid) launch_fint_gather(h->stream, h->N, h->inc(), h->d_fbuf, h->d_fint);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

extern "C" int tlfea_t10_get_n_elem(tlfea_t10_t h) { return h ? h->E : -1; }
extern "C" int tlfea_ancf_b12_matrix(int kind, double L, double W, double H, double* out_colmajor) {
  (void)H;  // the node reference points lie at w = 0: H does not enter B (cpu_utils.cc:125-188, 211-420)
  if (kind != 3243 && kind != 3443) return fail("tlfea_ancf_b12_matrix: kind must be 3243 or 3443");
  if (!out_colmajor) return fail("tlfea_ancf_b12_matrix: null output");
  if (!ancf::B_inv(kind == 3243 ? 8 : 16, L, W, out_colmajor)) return fail("tlfea_ancf_b12_matrix: singular B matrix");
  return 0;
}

extern "C" int tlfea_elem_dims(tlfea_t10_t h, int* S, int* Q) {
  if (!h) return fail("null handle");
  *S = h->S;
  *Q = h->Q;
  return 0;
}
extern "C" int tlfea_t10_get_n_coef(tlfea_t10_t h) { return h ? h->N : -1; }
extern "C" int tlfea_t10_get_n_constraint(tlfea_t10_t h) { return h ? h->n_constraint : -1; }
extern "C" int tlfea_t10_is_constraint_setup(tlfea_t10_t h) { return h && h->is_constraints_setup; }

extern "C" int tlfea_t10_mass_csr_nnz(tlfea_t10_t h, int* nnz) {
  if (!h || !nnz) return fail("null argument");
  *nnz = h->is_csr_setup ? h->nnz_mass : 0;
  return 0;
}
extern "C" int tlfea_t10_retrieve_mass_csr(tlfea_t10_t h, int* offsets, int* columns, double* values) {
  if (!h) return fail("null handle");
  if (!h->is_csr_setup) {
    std::fill(offsets, offsets + h->N + 1, 0);
    return 0;
  }
  if (h->nnz_mass == h->nnz_coef) {
    std::copy(h->h_off.begin(), h->h_off.end(), offsets);
    std::copy(h->h_cols.begin(), h->h_cols.end(), columns);
    HIP_TRY(hipMemcpy(values, h->d_mval, (size_t)h->nnz_coef * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  }
  // the internal adjacency also holds the pairs coupled by constraint rows; the mass CSR is the element part only
  std::vector<double> mv((size_t)h->nnz_coef);
  HIP_TRY(hipMemcpy(mv.data(), h->d_mval, mv.size() * sizeof(double), hipMemcpyDeviceToHost));
  int o = 0;
  for (int i = 0; i < h->N; i++) {
    offsets[i] = o;
    for (int k = h->h_off[i]; k < h->h_off[i + 1]; k++)
      if (!h->h_extra[k]) {
        columns[o] = h->h_cols[k];
        values[o++] = mv[k];
      }
  }
  offsets[h->N] = o;
  return 0;
}
extern "C" int tlfea_t10_retrieve_internal_force(tlfea_t10_t h, double* f) { D2H(f, h->d_fint, 3 * h->N); return 0; }
extern "C" int tlfea_t10_retrieve_external_force(tlfea_t10_t h, double* f) { D2H(f, h->d_fext, 3 * h->N); return 0; }
extern "C" int tlfea_t10_retrieve_position(tlfea_t10_t h, double* x, double* y, double* z) {
  D2H(x, h->d_x, h->N); D2H(y, h->d_y, h->N); D2H(z, h->d_z, h->N);
  return 0;
}
extern "C" int tlfea_t10_retrieve_p_from_f(tlfea_t10_t h, double* P) {
  if (!h->d_P) return fail("CalcP has not been called");
  D2H(P, h->d_P, (size_t)h->E * h->Q * 9);
  return 0;
}
extern "C" int tlfea_t10_retrieve_deformation_gradient(tlfea_t10_t h, double* F) {
  if (!h->d_F) return fail("CalcP has not been called");
  D2H(F, h->d_F, (size_t)h->E * h->Q * 9);
  return 0;
}
extern "C" int tlfea_t10_retrieve_dndu_pre(tlfea_t10_t h, double* g) { D2H(g, h->d_gradN, (size_t)h->E * h->Q * 3 * h->S); return 0; }
extern "C" int tlfea_t10_retrieve_detj(tlfea_t10_t h, double* d) { D2H(d, h->d_detJ, (size_t)h->E * h->Q); return 0; }
extern "C" int tlfea_t10_retrieve_connectivity(tlfea_t10_t h, int* c) { D2H(c, h->d_conn, (size_t)h->E * h->S); return 0; }
extern "C" int tlfea_t10_retrieve_constraint_data(tlfea_t10_t h, double* c) {
  if (!h->is_constraints_setup) return fail("constraint is not set up");
  if (h->n_constraint) D2H(c, h->d_cons, h->n_constraint);
  return 0;
}
extern "C" int tlfea_t10_retrieve_constraint_jac_csr(tlfea_t10_t h, int* offsets, int* columns, double* values) {
  if (!h->is_constraints_setup) return fail("constraint is not set up");
  if (h->cons_mode == 2) {  // RetrieveConstraintJacobianCSRToCPU (ANCF3243Data.cuh:1056-1091)
    std::copy(h->h_joff.begin(), h->h_joff.end(), offsets);
    std::copy(h->h_jcol.begin(), h->h_jcol.end(), columns);
    std::copy(h->h_jval.begin(), h->h_jval.end(), values);
    return 0;
  }
  for (int k = 0; k < h->n_constraint; k++) {  // FEAT10Data.cu:443-459
    offsets[k] = k;
    columns[k] = h->h_fixed[k / 3] * 3 + k % 3;
    values[k] = 1.0;
  }
  offsets[h->n_constraint] = h->n_constraint;
  return 0;
}
extern "C" int tlfea_t10_retrieve_constraint_jact_csr(tlfea_t10_t h, int* offsets, int* columns, double* values) {
  if (!h->is_constraints_setup) return fail("constraint is not set up");
  const int rows = 3 * h->N;
  if (h->cons_mode == 2) {
    std::copy(h->h_jtoff.begin(), h->h_jtoff.end(), offsets);
    std::copy(h->h_jtcol.begin(), h->h_jtcol.end(), columns);
    std::copy(h->h_jtval.begin(), h->h_jtval.end(), values);
    return 0;
  }
  std::fill(offsets, offsets + rows + 1, 0);
  for (int k = 0; k < h->n_constraint; k++) offsets[h->h_fixed[k / 3] * 3 + k % 3 + 1]++;
  for (int r = 0; r < rows; r++) offsets[r + 1] += offsets[r];
  std::vector<int> cur(offsets, offsets + rows);
  for (int k = 0; k < h->n_constraint; k++) {  // slot order: ascending constraint id (deterministic)
    const int r = h->h_fixed[k / 3] * 3 + k % 3;
    columns[cur[r]] = k;
    values[cur[r]++] = 1.0;
  }
  return 0;
}
extern "C" int tlfea_t10_write_output_vtk(tlfea_t10_t h, const char* filename) {
  std::vector<double> x(h->N), y(h->N), z(h->N);
  TRY(tlfea_t10_retrieve_position(h, x.data(), y.data(), z.data()));
  std::ofstream out(filename);
  if (!out) return fail(std::string("cannot open ") + filename);
  out << "# vtk DataFile Version 3.0\nT10 mesh output\nASCII\nDATASET UNSTRUCTURED_GRID\n";
  out << "POINTS " << h->N << " float\n";
  for (int i = 0; i < h->N; i++) out << x[i] << " " << y[i] << " " << z[i] << "\n";
  out << "CELLS " << h->E << " " << h->E * 11 << "\n";
  for (int e = 0; e < h->E; e++) {
    out << "10 ";
    for (int a = 0; a < kNN; a++) out << h->h_conn[(size_t)a * h->E + e] << " ";
    out << "\n";
  }
  out << "CELL_TYPES " << h->E << "\n";
  for (int e = 0; e < h->E; e++) out << "24\n";
  return 0;
}
extern "C" const double* tlfea_t10_x12_device_ptr(tlfea_t10_t h) { return h->d_x; }
extern "C" const double* tlfea_t10_y12_device_ptr(tlfea_t10_t h) { return h->d_y; }
extern "C" const double* tlfea_t10_z12_device_ptr(tlfea_t10_t h) { return h->d_z; }
extern "C" double* tlfea_t10_external_force_device_ptr(tlfea_t10_t h) { return h->d_fext; }
extern "C" double* tlfea_t10_constraint_device_ptr(tlfea_t10_t h) { return h->d_cons; }
