// data_handle.h -- the data object behind tlfea_t10_t (any element kind; its C-ABI is data_api.hip) and what of the units
// beside it (loads_api.hip, obstacle_api.hip) the rest of the host code calls.  Private to csrc/.
#pragma once
#include "api_common.h"
#include "t10_load_host.h"

// =================================================================================================
struct tlfea_t10_s {  // any element type; the name is kept for the ABI's first element type
  int kind = tlfea::kT10, S = tlfea::kNN, Q = tlfea::kNQ, nn = tlfea::kNN;  // shape functions, force QPs, nodes per element
  int n_nodes = 0;                             // mesh nodes (== N for T10, N/4 for the ANCF types)
  int E = 0, N = 0, Epad = 0;
  // ANCF set-up data (host): per-element dimensions, (B^T)^-1 column-major, force and mass rules
  std::vector<double> Lv, Wv, Hv, Binv;
  std::vector<double> fr[6], mr[6];  // gauss xi/eta/zeta, weight xi/eta/zeta
  int n_constraint = 0, n_fixed = 0;
  hipStream_t stream = nullptr;  // default stream, as the reference
  // mesh + state
  int* d_conn = nullptr;
  double *d_x = nullptr, *d_y = nullptr, *d_z = nullptr, *d_xt = nullptr, *d_yt = nullptr, *d_zt = nullptr;
  double *d_qx = nullptr, *d_qy = nullptr, *d_qz = nullptr;
  double h_qw[tlfea::kMaxQ] = {0};
  double *d_gradN = nullptr, *d_gradN_t = nullptr, *d_detJ = nullptr;
  double *d_F = nullptr, *d_P = nullptr, *d_Fdot = nullptr, *d_Pvis = nullptr;  // lazily, CalcP only
  double *d_fbuf = nullptr, *d_fint = nullptr, *d_fext = nullptr;
  tlfea::Material mat{tlfea::kSVK, 0, 0, 0, 0, 0, 0, 0, 0};
  double E_mod = 0, nu = 0;
  // per-element materials (tlfea_t10_set_element_materials): null d_emat = one material (mat) for every element.  While
  // a table is set, mat.model is the table's model and mat_saved the uniform material that ClearElementMaterials restores
  double* d_emat = nullptr;         // [E][kEmRec], tlfea_internal.h
  int n_mat = 0;
  bool emat_damp = false;           // some entry has eta or lamd != 0
  std::vector<double> h_table;      // [n_mat][kEmRec] (slot kEmRhoM: the entry's density)
  std::vector<int> h_eid;           // [E]
  std::vector<double> h_rho_mass;   // [E] density each element's share of the mass matrix was assembled with
  bool mass_pe = false;             // the mass matrix was assembled from h_rho_mass under a table
  tlfea::Material mat_saved{tlfea::kSVK, 0, 0, 0, 0, 0, 0, 0, 0};
  // rigid obstacles (tlfea_t10_set_obstacles): obs.n == 0 = none -- nothing allocated, nothing launched
  tlfea::ObstacleList obs{};
  std::vector<double> h_surf_w;     // [N] surface weight of every node (built once per mesh, on first use)
  std::vector<int> h_surf;          // the nodes of weight > 0, ascending: the obstacle kernels' work list
  int* d_ob_node = nullptr;
  double *d_ob_w = nullptr, *d_ob_f = nullptr, *d_ob_blk = nullptr, *d_ob_fk = nullptr, *d_ob_res = nullptr;
  int ob_fk_cap = 0;                // obstacles d_ob_fk has room for
  // field obstacles (tlfea_set_field_obstacles, DESIGN 3e''): obs.o[0 .. ob_na) are the analytic obstacles and
  // obs.o[ob_na .. obs.n) the fields, each list with its own index space; the samples (d_fld_V) and the descriptors
  // (d_fld [kMaxObstacles], host copy h_fld) live in device memory
  int ob_na = 0;
  std::vector<tlfea_field_obstacle> fld;
  std::vector<double*> d_fld_V;
  tlfea::FieldDev* d_fld = nullptr;
  tlfea::FieldDev h_fld[tlfea::kMaxObstacles] = {};
  // the same list on an ANCF object (tlfea_ancf_set_obstacles, DESIGN 3e'): sample-point tables and element-owned buffers
  // (AncfObsView, tlfea_internal.h); d_ao_fc [N][3] the contact force per coefficient, d_ao_pts [E][32][5] the footprint
  int *d_ao_cls = nullptr, *d_ao_touched = nullptr;
  double *d_ao_sval = nullptr, *d_ao_w = nullptr, *d_ao_cbuf = nullptr, *d_ao_blk = nullptr, *d_ao_fk = nullptr,
         *d_ao_fc = nullptr, *d_ao_pts = nullptr;
  std::vector<double> h_ao_w;       // [E][32] sample-point weights (built once per mesh, on first use)
  std::vector<int> h_ao_cls;
  std::vector<double> h_ao_sval;
  // distributed loads: none set = nothing allocated, nothing launched.  d_ld_fc [N][3] the constant part
  // (M a + the traction vector d_ld_tr), rebuilt by the next gradient evaluation while ld_const_dirty; d_ld_f [N][3] the
  // total load of the last gradient evaluation; the rest is AncfLoadView's (tlfea_internal.h)
  struct SurfaceLoad {
    int kind, face;
    double value[3], scale;
    std::vector<int> elems;
  };
  bool ld_have_a = false, ld_const_dirty = false;
  double ld_a[3] = {0, 0, 0};
  std::vector<SurfaceLoad> ld_list;
  int ld_n_trac = 0, ld_n_press = 0;
  double *d_ld_fc = nullptr, *d_ld_tr = nullptr, *d_ld_f = nullptr, *d_ld_lbuf = nullptr, *d_ld_tab = nullptr,
         *d_ld_qw = nullptr, *d_ld_pe = nullptr;
  int *d_ld_cls = nullptr, *d_ld_mask = nullptr;
  // surface loads on a T10 object (DESIGN 3h'): ld_list holds boundary-face indices in `elems`; the pressure's loaded faces
  // (ascending) own the rows of d_ld_lbuf [n][6][3], d_ld_pe [n] their effective pressure, d_ld_fnodes [n][6] their nodes,
  // d_ld_foff / d_ld_fslot the node-to-row CSR of the gather
  tlfea::t10load::BoundaryFaces bf;
  bool bf_built = false;
  std::vector<int> h_ld_lf;         // the loaded faces, ascending
  int *d_ld_fnodes = nullptr, *d_ld_foff = nullptr, *d_ld_fslot = nullptr;
  bool loads_on() const { return ld_have_a || !ld_list.empty(); }
  // stress recovery (tlfea_t10_calc_stress): allocated on first use, read by no solver
  double *d_st_pts = nullptr, *d_st_erec = nullptr, *d_st_contrib = nullptr, *d_st_nodal = nullptr,
         *d_st_part = nullptr, *d_st_tot = nullptr, *d_st_vel = nullptr;
  double st_tot[5] = {0, 0, 0, 0, 0};
  bool st_valid = false, st_pts_valid = false;  // a calc_stress has run | its point stresses were asked for
  int *d_st_noff = nullptr, *d_st_nel = nullptr;  // ANCF (DESIGN 3f'): elements of every MESH node, ascending (n_nodes + 1 | E nn)
  bool ancf_mass = false;                         // ANCF: d_mval holds an assembled mass matrix (the kinetic energy's condition)
  double ancf_mass_rho0 = 0.0;                    // ... and the density it was assembled with (the adjoint's density slot, 3j')
  double* d_sn_rho = nullptr;                     // ANCF adjoint: [N] terms of the density slot (ancf_rho_terms_kernel)
  // recovered stress (tlfea_t10_recover_stress, DESIGN 3f''): allocated on first use, read by no solver.  d_rc_rec
  // [E][kRecoveryRec], d_rc_nodal [N][7], d_rc_err [3][Epad], principal values d_rc_pn [N][4] / d_rc_pe [E][4] and
  // directions d_rc_dn [N][9] / d_rc_de [E][9]; d_rc_pts [E][5][6] holds the point values of the _from_points hook
  double *d_rc_rec = nullptr, *d_rc_nodal = nullptr, *d_rc_err = nullptr, *d_rc_part = nullptr, *d_rc_tot = nullptr,
         *d_rc_pn = nullptr, *d_rc_pe = nullptr, *d_rc_dn = nullptr, *d_rc_de = nullptr, *d_rc_pts = nullptr;
  double rc_tot[4] = {0, 0, 0, 0};  // eta^2, n^2, eta_rel, clamped elements
  bool rc_valid = false, rc_principal = false, rc_directions = false;
  // material sensitivities (tlfea_t10_material_sensitivity): allocated on first use.  d_sn_sens [4][Epad],
  // d_sn_out [n_mat][P + 1]; under a table the ascending element list of every material (d_sn_idx [E], concatenated),
  // its chunks (d_sn_blk) and the first chunk of every material (d_sn_boff), rebuilt when `gen` has moved on
  double *d_sn_sens = nullptr, *d_sn_part = nullptr, *d_sn_out = nullptr, *d_sn_w = nullptr, *d_sn_u = nullptr,
         *d_sn_pe = nullptr;
  int *d_sn_idx = nullptr, *d_sn_boff = nullptr;
  int2* d_sn_blk = nullptr;
  int sn_nb = 0, sn_part_cap = 0, sn_out_cap = 0;
  long sn_gen = -1;
  // shape sensitivities (tlfea_t10_shape_sensitivity): allocated on first use.  d_sh_rows [10][Epad][3] the
  // element rows, d_sh_out [N][3] the gathered cotangent of the host form
  double *d_sh_rows = nullptr, *d_sh_out = nullptr;
  // constraints
  double* d_cons = nullptr;
  int *d_fixed = nullptr, *d_fixed_slot = nullptr;
  std::vector<int> h_fixed;
  // constraint mode: 0 none, 1 fixed coefficients (SetNodalFixed), 2 general linear rows (SetLinearConstraintsCSR);
  // mode 2 keeps J (rows = constraints) and J^T (rows = DOFs, entries in ascending constraint id) in CSR
  int cons_mode = 0;
  std::vector<int> h_joff, h_jcol, h_jtoff, h_jtcol;
  std::vector<double> h_jval, h_jtval, h_rhs;
  int *d_joff = nullptr, *d_jcol = nullptr, *d_jtoff = nullptr, *d_jtcol = nullptr;
  double *d_jval = nullptr, *d_jtval = nullptr, *d_rhs = nullptr;
  // entries of the coefficient adjacency that exist only through a constraint row (not part of the mass pattern)
  std::vector<char> h_extra;
  int nnz_mass = 0;
  // sparsity (host copies are kept: the solver and the retrieve calls need them)
  std::vector<int> h_conn, h_off, h_cols, h_n2e_off, h_n2e;
  double h_q[3][tlfea::kNQ] = {{0}};  // T10 quadrature points (host copy: shape-function table of the element-wise inertia term)
  bool fbuf_valid = true;      // d_fbuf holds the force rows of the last residual evaluation (false after a solver
                               // evaluation on the interleaved-row path: d_fint itself is then current)
  double mass_rho0 = -1.0;     // density the mass matrix was assembled with (CalcMassMatrix); < 0: not assembled
  std::vector<double> h_X0;  // coordinates handed to Setup (x | y | z): the Morton order of the fused assembly's row groups
  int *d_off = nullptr, *d_cols = nullptr, *d_n2e_off = nullptr, *d_n2e = nullptr, *d_n2e_pos = nullptr,
      *d_diagpos = nullptr;
  double* d_mval = nullptr;
  int nnz_coef = 0, maxdeg = 0;
  // bumped by every setter that changes what a captured launch has baked in (material scalars travel by value, the
  // fixed-node buffers are re-allocated by UpdateNodalFixed): cached hipGraphs carry the value they were captured at
  long gen = 0;
  // bumped by CalcDnDuPre: the solver's affine-form cache (vertex gradients, det J, the 'all elements straight-sided'
  // decision) was derived from the grad N / det J of one call and must follow a re-referencing
  long geom_gen = 0;
  bool is_setup = false, is_constraints_setup = false, is_csr_setup = false, is_j_csr_setup = false,
       is_cj_csr_setup = false, have_dndu = false;

  tlfea::ElemView view() const {
    tlfea::ElemView v;
    v.E = E; v.N = N; v.Epad = Epad; v.S = S; v.Q = Q;
    v.conn = d_conn; v.x = d_x; v.y = d_y; v.z = d_z;
    v.gradN = d_gradN; v.gradN_t = d_gradN_t; v.detJ = d_detJ;
    for (int q = 0; q < tlfea::kMaxQ; q++) v.qw[q] = h_qw[q];
    return v;
  }
  tlfea::Incidence inc() const { return tlfea::Incidence{d_n2e_off, d_n2e, d_n2e_pos, d_off, d_cols, d_diagpos}; }
};

namespace tlfea {

inline AncfObsView ancf_obs_view(tlfea_t10_t h) {
  return AncfObsView{h->E, h->S, h->d_conn, h->d_ao_cls, h->d_ao_sval, h->d_ao_w, h->d_ao_cbuf, h->d_ao_blk,
                     h->d_ao_fk, h->d_ao_touched};
}

inline bool mass_assembled(tlfea_t10_t h) { return h->kind == kT10 ? h->mass_rho0 >= 0.0 : h->ancf_mass; }

// loads_api.hip: the boundary faces of a T10 mesh (built once, kept in the handle) and the traction vector of the loads
// set, which follow the reference geometry
void boundary_faces_build(tlfea_t10_t h);
int loads_build_traction(tlfea_t10_t h);
int t10_loads_build_traction(tlfea_t10_t h);
// obstacle_api.hip
int ancf_points_build(tlfea_t10_t h);
// the reference geometry of a T10 object has moved (tlfea_t10_set_reference_positions): surface weights again from h_X0
int t10_surface_refresh(tlfea_t10_t h);

}  // namespace tlfea
