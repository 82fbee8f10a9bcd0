/* tlfea_c.h -- C-ABI of the MI355X-native Total-Lagrangian element engine (libtlfea_hip.so).
 *
 * This is the drop-in boundary for the T10 hot path of uwsbel/Total-Lagrangian-FEA.  The reference
 * has no FFI: its boundary is the C++ class surface the drivers in lib_bin/ call
 * (GPU_FEAT10_Data, SyncedNewtonSolver).  Every entry point below replaces one member function of
 * those classes (cited as file:line, paths relative to the reference root) with a handle-based
 * `extern "C"` function taking plain pointers and sizes.  The header-only C++ facade in
 * total-lagrangian-fea_amd/host/ re-creates the reference class names on top of this ABI, and
 * total-lagrangian-fea_amd/__init__.py binds it with ctypes.
 *
 * Conventions
 *   - all floating point is fp64, all indices int32, zero based;
 *   - host pointers unless the name says `_device_ptr`;
 *   - every function returns 0 on success, non-zero on failure (tlfea_last_error() gives text);
 *     API misuse mirrors the reference: message on stderr + early return (non-zero here);
 *   - one handle <-> one GPU (the current HIP device at create time), default stream, blocking,
 *     not thread-safe (as the reference: FEAT10Data.cu:291,311,332);
 *   - ownership: the data handle owns every device buffer until tlfea_t10_destroy(); a solver
 *     handle borrows the data handle, which must outlive it (SyncedNewton.cuh:37-46).
 *   - layouts handed across the ABI are the reference's: connectivity column-major E x 10
 *     (FEAT10Data.cuh:36-39), grad-N blocks 10x3 column-major per (elem,qp) (:41-45), F/P 3x3
 *     column-major per (elem,qp) (:114-158), forces/velocities xyz-interleaved per node.
 */
#ifndef TLFEA_C_H
#define TLFEA_C_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tlfea_t10_s *tlfea_t10_t;       /* GPU_FEAT10_Data   (FEAT10Data.cuh:19)   */
typedef struct tlfea_newton_s *tlfea_newton_t; /* SyncedNewtonSolver (SyncedNewton.cuh:35) */

/* SyncedNewtonParams (SyncedNewton.cuh:29-33) -- identical field order. */
typedef struct {
  double inner_atol, inner_rtol, outer_tol, rho;
  int max_outer, max_inner;
  double time_step;
} tlfea_newton_params;

/* Linear-solve options.  The reference calls cuDSS (sparse Cholesky, SyncedNewton.cu:995-1029,
 * 1103-1114); this engine solves the same SPD system H dv = -g on the device: by default with CG in fp64 on H,
 * preconditioned by a two-level p-multigrid cycle (T10) or a Chebyshev polynomial of the block-Jacobi-scaled
 * operator (all kinds), both streaming a scaled fp16 copy of H with fp32 work vectors; method = 1 selects the sparse
 * direct solve (the engine's multifrontal Cholesky: analysis once per mesh, re-factorisation + solve per call, as the
 * reference drives cuDSS).  rel_tol is on ||r||/||b|| of the fp64 system. */
typedef struct {
  double rel_tol;    /* default 1e-12 */
  int max_iter;      /* default 20000 (outer CG iterations) */
  int check_every;   /* outer iterations between host convergence checks (default 25) */
  int cheb_degree;   /* degree of the Chebyshev polynomial of D^-1 H used as preconditioner; 1 = plain block-Jacobi;
                        0 (default) = auto = 24 */
  double cheb_kappa; /* the polynomial targets [lmax/kappa, lmax] of D^-1 H; <= 1 (default 0) = auto by degree
                        (400 / 800 / 1600 for degree < 14 / < 22 / above) */
  int cheb_bits;     /* storage precision of the matrix the polynomial streams: 64 = H itself; 32 / 16 = a symmetrically
                        scaled fp32 / fp16 block copy, and on one GPU the polynomial's recurrence then runs in fp32
                        (the outer CG, its residual and its convergence test stay fp64 on H);
                        0 (default) = auto = 16 */
  int precond;       /* 0 (default) = auto, 1 = Chebyshev polynomial of block-Jacobi, 2 = two-level p-multigrid (T10 on one
                        GPU: quadratic tets -> their vertex mesh, Galerkin coarse operator, polynomial smoothers and
                        coarse solve; auto picks it wherever it exists) */
  int method;        /* 0 (default) = preconditioned CG; 1 = sparse direct (single GPU) */
  int on_unconverged;/* a CG solve that ends above rel_tol (max_iter reached, or breakdown after the interval widenings):
                        0 (default) = the call fails, nothing is applied to v and x (the reference aborts when cuDSS
                        fails, SyncedNewton.cu:995-1029); 1 = accept the iterate (experiments with a capped iteration
                        count) -- tlfea_newton_get_linsolve_status reports it */
} tlfea_linsolve_opts;

const char *tlfea_last_error(void);
int tlfea_version(void);
/* number of visible HIP devices; <=0 means the product path cannot run (it never falls back to CPU) */
int tlfea_device_count(void);

/* ---- GPU_FEAT10_Data ------------------------------------------------------------------------ */
/* ctor (FEAT10Data.cuh:377-380) + Initialize() (:382-433) */
int tlfea_t10_create(int n_elem, int n_nodes, tlfea_t10_t *out);
/* Destroy() (:714-779) */
int tlfea_t10_destroy(tlfea_t10_t h);
/* Setup(tet5pt_x,y,z,w, x12,y12,z12, element_connectivity) (:435-533); conn column-major E x 10 */
int tlfea_t10_setup(tlfea_t10_t h, const double *qx, const double *qy, const double *qz,
                    const double *qw, const double *x, const double *y, const double *z,
                    const int *conn_colmajor);
int tlfea_t10_set_density(tlfea_t10_t h, double rho0);                       /* :538-546 */
int tlfea_t10_set_damping(tlfea_t10_t h, double eta_damp, double lambda_damp); /* :553-563 */
int tlfea_t10_set_svk_select(tlfea_t10_t h);                                   /* SetSVK() :568-587 */
int tlfea_t10_set_svk(tlfea_t10_t h, double E, double nu);                     /* SetSVK(E,nu) :594-611 */
int tlfea_t10_set_mooney_rivlin(tlfea_t10_t h, double mu10, double mu01, double kappa); /* :618-634 */

/* Per-element materials (no reference counterpart).  A table of n_mat entries (1..256) and one id per element
 * (elem_material[E], each in 0..n_mat-1); `model` (0 SVK: E, nu; 1 Mooney-Rivlin: mu10, mu01, kappa) applies to every
 * entry.  After Setup only, T10 handles only.  Stiffness and damping take effect at the next evaluation, the densities
 * at the next CalcMassMatrix (the mass matrix assembled before keeps its densities).  While a table is set, the uniform
 * setters (set_svk, set_mooney_rivlin, set_density, set_damping) fail, and so do tlfea_newton_set_halo and
 * tlfea_newton_set_interface.  clear returns the object to its uniform material; a mass matrix assembled under the
 * table is dropped (CalcMassMatrix again).  get: n_mat (0 = uniform) and, when elem_material is not null and a table
 * is set, the E ids. */
typedef struct { double E, nu, mu10, mu01, kappa, rho0, eta, lamd; } tlfea_material_entry;
int tlfea_t10_set_element_materials(tlfea_t10_t h, int model, int n_mat, const tlfea_material_entry *table,
                                    const int *elem_material, int n_elem);
int tlfea_t10_clear_element_materials(tlfea_t10_t h);
int tlfea_t10_get_element_materials(tlfea_t10_t h, int *n_mat, int *elem_material);

/* Rigid analytic obstacles (no reference counterpart).  Up to 16 half-spaces (kind 0: point p, outward unit
 * normal n) and solid spheres (kind 1: centre p, radius) per T10 object, in implicit penalty contact with the surface
 * nodes: every solver that evaluates the gradient (Newton, direct Newton, AdamW, Nesterov) adds the contact gradient, and
 * Newton its 3x3 Hessian blocks.  stiffness: kappa in Pa/m (per unit surface area and penetration); friction: mu
 * (regularised Coulomb with the normal force of the start of the step); eps_v: friction regularisation velocity; vel:
 * obstacle velocity (friction only).  After Setup only.  While obstacles are set, tlfea_vbd_solve, tlfea_newton_set_halo
 * and tlfea_newton_set_interface fail.  update moves obstacle k between steps; clear removes all.
 * get_obstacle_forces: the contact force on every node (3N, the layout of f_ext) of the last gradient evaluation;
 * get_obstacle_resultant: obstacle k's total force on the mesh (out[0..2]) and its nodes in contact (out[3]);
 * get_surface_weights: the area share of every node (N, 0 inside the mesh). */
typedef struct {
  int kind;         /* 0 half-space, 1 sphere */
  double p[3];      /* point on the plane | centre */
  double n[3];      /* outward unit normal (half-space) */
  double radius;    /* sphere */
  double vel[3];    /* obstacle velocity (friction only) */
  double stiffness; /* kappa, Pa/m */
  double friction;  /* mu >= 0 */
  double eps_v;     /* friction regularisation velocity, m/s */
} tlfea_obstacle;
int tlfea_t10_set_obstacles(tlfea_t10_t h, const tlfea_obstacle *list, int n);
int tlfea_t10_update_obstacle(tlfea_t10_t h, int k, const tlfea_obstacle *o);
int tlfea_t10_clear_obstacles(tlfea_t10_t h);
int tlfea_t10_get_obstacle_forces(tlfea_t10_t h, double *f);
int tlfea_t10_get_obstacle_resultant(tlfea_t10_t h, int k, double out[4]);
int tlfea_t10_get_surface_weights(tlfea_t10_t h, double *w);
/* The same obstacles on ANCF-3243 / ANCF-3443 objects (DESIGN 3e'): contact is evaluated at 32 sample points on the
 * faces of every element (shell: the faces zeta = -1, +1 with the 4 x 4 Gauss rule; beam: the four side faces with
 * 4 x 2 Gauss points; no points on a shell's edge faces or a beam's end caps) and spread to the element's coefficients
 * through the shape functions.  After Setup and CalcDsDuPre only; the limits, checks and refusals of the T10 entry points
 * apply (which keep refusing ANCF handles, as these refuse T10 handles).
 * get_obstacle_forces: the contact force on every coefficient (3 n_coef, the layout of f_ext) of the last gradient
 * evaluation; get_obstacle_resultant: obstacle k's force on the mesh (out[0..2]) and its sample points in contact
 * (out[3]); get_surface_points: the weight of every sample point (E * 32: quadrature weight x reference surface
 * Jacobian, summing to the sampled area); retrieve_contact_points: E * 32 * 5 doubles, per point x y z, the smallest
 * gap over the obstacles and the normal pressure sum_k kappa_k <-d_k> at the current coordinates (computed by this call:
 * the same as at the last gradient evaluation unless the positions were changed since). */
int tlfea_ancf_set_obstacles(tlfea_t10_t h, const tlfea_obstacle *list, int n);
int tlfea_ancf_update_obstacle(tlfea_t10_t h, int k, const tlfea_obstacle *o);
int tlfea_ancf_clear_obstacles(tlfea_t10_t h);
int tlfea_ancf_get_obstacle_forces(tlfea_t10_t h, double *f);
int tlfea_ancf_get_obstacle_resultant(tlfea_t10_t h, int k, double out[4]);
int tlfea_ancf_get_surface_points(tlfea_t10_t h, double *w);
int tlfea_ancf_retrieve_contact_points(tlfea_t10_t h, double *out);
/* Field obstacles (no reference counterpart; DESIGN 3e''), any handle: a rigid obstacle given as a regular grid of
 * signed-distance samples (negative inside the body) with a rigid pose, in implicit contact with T10 surface nodes and
 * ANCF sample points through the model of the analytic obstacles, the interpolated gap phi in the place of the distance
 * and its gradient G in the place of the normal: force kappa w <-phi> G, Hessian block kappa w G G^T, friction from
 * G / |G| and kappa w <-phi> |G| at the start of the step.  values[k]: nx * ny * nz doubles, V[(iz * ny + iy) * nx + ix]
 * at origin + spacing * (ix, iy, iz) in the obstacle's frame; pos and rot (row-major, frame -> world) place the frame.
 * Interpolation is the uniform quadratic B-spline (C1); a point is covered iff 0.5 <= (s_a - origin_a) / spacing <=
 * n_a - 1.5 on every axis, s = rot^T (x - pos), and an obstacle contributes exactly nothing to a point it does not cover.
 * Accepted only if every sample is finite and every sample of the two outermost layers of each axis is > 0 (a closed body
 * well inside its grid: n_a >= 5; at most 2^27 samples), rot is orthonormal to 1e-12 with determinant +1, spacing > 0.
 * The samples are copied to the device; a call that fails leaves the previous field list as it was.
 * Analytic and field obstacles together number at most 16; each list keeps its own
 * index space, setting or clearing one leaves the other in place, and tlfea_*_get_obstacle_forces returns the total of
 * both.  After Setup (ANCF: and CalcDsDuPre).  The refusals of the analytic obstacles apply (VBD, halo, interface).
 * update: pose, vel, stiffness, friction, eps_v of field k; the grid must be the stored one and the samples are kept.
 * get_field_obstacle_resultant: field k's force on the mesh (out[0..2]) and its nodes / sample points in contact (out[3]).
 * tlfea_sdf_from_triangles (no handle): the signed distance of the closed, consistently oriented triangle surface
 * (verts [n_verts][3], tris [n_tris][3]) at the nx * ny * nz grid points, computed on the device into `values`; negative
 * inside, for either orientation.  At most 2^24 triangles.  Refuses indices out of range, a triangle of zero area and a surface some directed edge
 * of which does not occur exactly once with its reverse exactly once. */
typedef struct {
  int nx, ny, nz;
  double origin[3];
  double spacing;
  double pos[3];
  double rot[9];
  double vel[3];
  double stiffness, friction, eps_v;
} tlfea_field_obstacle;
int tlfea_set_field_obstacles(tlfea_t10_t h, const tlfea_field_obstacle *list, const double *const *values, int n);
int tlfea_update_field_obstacle(tlfea_t10_t h, int k, const tlfea_field_obstacle *o);
int tlfea_clear_field_obstacles(tlfea_t10_t h);
int tlfea_get_field_obstacle_resultant(tlfea_t10_t h, int k, double out[4]);
int tlfea_sdf_from_triangles(const double *verts, int n_verts, const int *tris, int n_tris, int nx, int ny, int nz,
                             const double origin[3], double spacing, double *values);
/* Distributed loads (no reference counterpart).  They live beside f_ext, not in it: every gradient evaluation
 * (Newton, direct Newton, AdamW, Nesterov) does g -= f_load(x), and tlfea_t10_set_external_force / retrieve_external_force
 * keep their meaning.  Nothing is allocated or launched while no load is set.
 * Body acceleration a (gravity), any handle: f_i = sum_j M_ij a_j with a_j = a on position coefficients (every
 * coefficient of a T10 mesh, coefficient 4 n of ANCF node n) and 0 on gradient coefficients, from the mass matrix on the
 * device; after CalcMassMatrix only, and rebuilt after a later CalcMassMatrix.
 * Surface loads, ANCF handles only, after Setup and CalcDsDuPre, at most 16: each applies to one face of a list of
 * elements (shell: zeta = -1, +1 -> face 0, 1; beam: eta = -1, +1, zeta = -1, +1 -> face 0..3, as the obstacle sample
 * points number them).  kind 0, dead traction value[0..2] (force per reference area, fixed direction), integrated with
 * the obstacle sample points of the face; kind 1, follower pressure value[0] (positive pushes against the outward normal
 * of the deformed face), integrated at the current coefficients with a 5 x 5 (shell) or 5 x 2 (beam) Gauss rule.  scale
 * multiplies the value; update_load_scale changes it between steps (ramps) without sending the list again.  An element
 * index outside 0..E-1, a face outside the kind's range and the same element twice in one load are refused.  The pressure
 * load stiffness is left out of the Hessian (it is unsymmetric; H stays SPD), so Newton converges linearly in that term.
 * set_surface_loads replaces the list (n = 0 removes it); clear_loads removes the list and the body acceleration.
 * While loads are set, tlfea_vbd_solve, tlfea_newton_set_halo and tlfea_newton_set_interface fail.
 * get_load_forces: the load on every coefficient (3 n_coef, the layout of f_ext) of the last gradient evaluation;
 * get_load_resultant: its sum over the position coefficients. */
#define TLFEA_MAX_LOADS 16
typedef struct {
  int kind;          /* 0 dead traction, 1 follower pressure */
  int face;          /* shell 0..1, beam 0..3 */
  double value[3];   /* traction vector | pressure in value[0] */
  double scale;      /* multiplies value */
  const int *elems;  /* element indices */
  int n_elems;
} tlfea_surface_load;
int tlfea_set_body_acceleration(tlfea_t10_t h, const double a[3]);
int tlfea_ancf_set_surface_loads(tlfea_t10_t h, const tlfea_surface_load *list, int n);
int tlfea_ancf_update_load_scale(tlfea_t10_t h, int k, double scale);
int tlfea_clear_loads(tlfea_t10_t h);
int tlfea_get_load_forces(tlfea_t10_t h, double *f);
int tlfea_get_load_resultant(tlfea_t10_t h, double out[3]);
/* Surface loads on the boundary faces of a T10 mesh (DESIGN 3h'), T10 handles only, after Setup.  A boundary face is a
 * 6-node triangle that belongs to exactly one tet; the faces are numbered in ascending (element, local face) order, and
 * this numbering is part of the interface.  get_boundary_faces: the count (null arrays: the count alone), per face its
 * element, its local face (0..3: the face of nodes 012, 013, 023, 123) and its six node ids (nodes: 6 * n_faces; corners,
 * then the mid-edge nodes 01 12 02), ordered so that the normal X_xi x X_eta points out of the mesh.
 * A load applies to a list of boundary faces: kind 0, dead traction value[0..2] (force per reference area, fixed
 * direction); kind 1, follower pressure value[0] (positive pushes against the outward normal of the deformed face),
 * integrated at the current positions.  Both use the 6-point triangle rule of degree 4, which is exact for the pressure
 * and for the traction on a straight-sided face.  scale multiplies the value; update_load_scale changes it between steps.
 * At most 16 loads; several pressures on one face add.  A face outside 0..n_faces-1, the same face twice in one load, an
 * unknown kind and a non-finite value or scale are refused.  set_surface_loads replaces the list (n = 0 removes it);
 * tlfea_clear_loads removes it and the body acceleration; get_load_forces and get_load_resultant include these loads.
 * The pressure load stiffness is left out of the Hessian, and tlfea_vbd_solve, tlfea_newton_set_halo and
 * tlfea_newton_set_interface fail while loads are set, as above. */
typedef struct {
  int kind;          /* 0 dead traction, 1 follower pressure */
  double value[3];   /* traction vector | pressure in value[0] */
  double scale;      /* multiplies value */
  const int *faces;  /* boundary-face indices */
  int n_faces;
} tlfea_t10_surface_load;
int tlfea_t10_get_boundary_faces(tlfea_t10_t h, int *n_faces, int *elem, int *local_face, int *nodes);
int tlfea_t10_set_surface_loads(tlfea_t10_t h, const tlfea_t10_surface_load *list, int n);
int tlfea_t10_update_load_scale(tlfea_t10_t h, int k, double scale);
/* Stress and energy recovery of T10 objects (no reference counterpart).  Works from the current positions and
 * the object's own data at any time after CalcDnDuPre; changes nothing a solver reads.  d_vel: DEVICE pointer to a
 * velocity (3N interleaved: what tlfea_*_velocity_guess_device_ptr returns) or NULL; with it a damped material's
 * Kelvin-Voigt stress is added (the P of the residual), and the kinetic energy and viscous power are formed (needs
 * CalcMassMatrix).  calc_stress_host takes the velocity from the host.  want_points != 0 also keeps the stresses of the
 * five Keast points.  Cauchy stresses are 6 doubles xx yy zz xy yz zx.  Element values are reference-volume-weighted means
 * over the points (von Mises of the mean stress; psi = elastic strain-energy density per reference volume; J = det F);
 * nodal stress is the element-volume-weighted mean of the incident elements' means, von Mises taken from that tensor.
 * get_energies: strain energy, kinetic energy 1/2 v.Mv, viscous power, reference volume, current volume.  A retrieve
 * before calc_stress is an error.  Every output is bitwise reproducible.  ANCF handles are refused. */
int tlfea_t10_calc_stress(tlfea_t10_t h, const double *d_vel /* device, 3N, or NULL */, int want_points);
int tlfea_t10_calc_stress_host(tlfea_t10_t h, const double *vel /* host, 3N, or NULL */, int want_points);
int tlfea_t10_retrieve_point_stress(tlfea_t10_t h, double *sigma /*E*5*6*/);
int tlfea_t10_retrieve_element_stress(tlfea_t10_t h, double *sigma /*E*6*/, double *von_mises /*E*/, double *psi /*E*/,
                                      double *J /*E*/, double *vol /*E*/); /* any may be NULL */
int tlfea_t10_retrieve_nodal_stress(tlfea_t10_t h, double *sigma /*N*6*/, double *von_mises /*N*/); /* either may be NULL */
int tlfea_t10_get_energies(tlfea_t10_t h, double out[5]);
double *tlfea_t10_nodal_stress_device_ptr(tlfea_t10_t h); /* N*7: sigma, von Mises per node; NULL before calc_stress */
/* mean ms over reps launches of: the point and element kernel, the nodal gather, the totals (profiling hook) */
int tlfea_t10_time_stress_kernels(tlfea_t10_t h, const double *d_vel, int want_points, int reps, double *out_ms3);
/* Recovered stress of T10 objects (no reference counterpart; DESIGN 3f'').  Works from the stored point stresses of the
 * last tlfea_t10_calc_stress(.., want_points = 1); changes nothing a solver reads and nothing of that stress recovery.
 *   recovered nodal stress  per element a field linear in the reference coordinates is fitted to the five point values by
 *                           unweighted least squares and evaluated at the ten nodes; node i takes the V_e-weighted mean of
 *                           these values over its elements in ascending order; von Mises of that tensor beside it
 *   principal stresses      of the recovered nodal tensors and of the element mean tensors: values = s1 >= s2 >= s3 |
 *                           (s1 - s3) / 2; directions = the unit eigenvectors of s1, s2, s3 as rows of a right-handed frame
 *                           (any orthonormal frame of the eigenspace at a multiple root)
 *   error indicator         e_q = the recovered field, interpolated with the shape functions, minus the point stress;
 *                           eta_e^2 = max(0, sum_q dV_q |e_q|^2), n_e^2 = sum_q dV_q |sigma_q|^2 with
 *                           |s|^2 = dev(s):dev(s) / (2 mu) + tr(s)^2 / (9 K), mu and K the small-strain moduli of the
 *                           element's material.  get_error_estimate: sum eta_e^2, sum n_e^2,
 *                           eta_rel = sqrt(eta^2 / (n^2 + eta^2)) (0 when both vanish), elements clamped at 0
 * want_directions implies want_principal.  recover_stress_from_points runs the same launches on point values given by
 * the caller (host, E*5*6; needs CalcDnDuPre, no calc_stress).  A retrieve before a recovery is an error, as is asking for
 * principal values or directions the last recovery did not compute.  Every output is bitwise reproducible.  ANCF handles
 * are refused. */
int tlfea_t10_recover_stress(tlfea_t10_t h, int want_principal, int want_directions);
int tlfea_t10_recover_stress_from_points(tlfea_t10_t h, const double *points /* host, E*5*6 */, int want_principal,
                                         int want_directions);
int tlfea_t10_retrieve_recovered_stress(tlfea_t10_t h, double *sigma /*N*6*/, double *von_mises /*N*/); /* either may be NULL */
int tlfea_t10_retrieve_principal_stress(tlfea_t10_t h, double *nodal_values /*N*4*/, double *nodal_directions /*N*9*/,
                                        double *element_values /*E*4*/, double *element_directions /*E*9*/); /* any may be NULL */
int tlfea_t10_retrieve_error_indicator(tlfea_t10_t h, double *eta2 /*E*/, double *n2 /*E*/); /* either may be NULL */
int tlfea_t10_get_error_estimate(tlfea_t10_t h, double out[4]);
double *tlfea_t10_recovered_stress_device_ptr(tlfea_t10_t h); /* N*7: sigma*, von Mises per node; NULL before a recovery */
/* mean ms over reps launches of: the element records, the nodal gather from them, the nodal gather straight from the
 * point blocks (the form not kept), the principal launches, the error indicator, its totals (profiling hook) */
int tlfea_t10_time_recovery_kernels(tlfea_t10_t h, int reps, double *out_ms6);
int tlfea_t10_set_external_force(tlfea_t10_t h, const double *f_ext, int n);   /* :636-646 (n must be 3N) */
int tlfea_t10_set_nodal_fixed(tlfea_t10_t h, const int *fixed_nodes, int n_fixed);    /* FEAT10Data.cu:728-749 */
int tlfea_t10_update_nodal_fixed(tlfea_t10_t h, const int *fixed_nodes, int n_fixed); /* FEAT10Data.cu:751-832 */
int tlfea_t10_update_positions(tlfea_t10_t h, const double *x, const double *y, const double *z, int n);          /* :671-685 */
int tlfea_t10_update_constraint_targets(tlfea_t10_t h, const double *x, const double *y, const double *z, int n); /* :687-701 */

int tlfea_t10_calc_dndu_pre(tlfea_t10_t h);            /* CalcDnDuPre        FEAT10Data.cu:284-292 */
int tlfea_t10_build_mass_csr_pattern(tlfea_t10_t h);   /* BuildMassCSRPattern FEAT10Data.cu:372-440 */
int tlfea_t10_calc_mass_matrix(tlfea_t10_t h);         /* CalcMassMatrix     FEAT10Data.cu:351-370 */
int tlfea_t10_calc_constraint_data(tlfea_t10_t h);     /* CalcConstraintData FEAT10Data.cu:335-349 */
int tlfea_t10_convert_to_csr_constraint_jac(tlfea_t10_t h);  /* FEAT10Data.cu:501-534 */
int tlfea_t10_convert_to_csr_constraint_jact(tlfea_t10_t h); /* FEAT10Data.cu:538-601 */
int tlfea_t10_calc_p(tlfea_t10_t h);                   /* CalcP              FEAT10Data.cu:307-312 */
int tlfea_t10_calc_internal_force(tlfea_t10_t h);      /* CalcInternalForce  FEAT10Data.cu:328-333 */

int tlfea_t10_get_n_elem(tlfea_t10_t h);
int tlfea_t10_get_n_coef(tlfea_t10_t h);
int tlfea_t10_get_n_constraint(tlfea_t10_t h);
int tlfea_t10_is_constraint_setup(tlfea_t10_t h); /* Get_Is_Constraint_Setup :785-787 */

/* Retrieve*ToCPU (FEAT10Data.cu:603-726,834-839); flat arrays in the reference's device layouts */
int tlfea_t10_mass_csr_nnz(tlfea_t10_t h, int *nnz);
int tlfea_t10_retrieve_mass_csr(tlfea_t10_t h, int *offsets /*N+1*/, int *columns /*nnz*/, double *values /*nnz*/);
int tlfea_t10_retrieve_internal_force(tlfea_t10_t h, double *f /*3N*/);
int tlfea_t10_retrieve_external_force(tlfea_t10_t h, double *f /*3N*/);
int tlfea_t10_retrieve_position(tlfea_t10_t h, double *x, double *y, double *z);
int tlfea_t10_retrieve_p_from_f(tlfea_t10_t h, double *P /*E*5*9*/);
int tlfea_t10_retrieve_deformation_gradient(tlfea_t10_t h, double *F /*E*5*9*/);
int tlfea_t10_retrieve_dndu_pre(tlfea_t10_t h, double *gradN /*E*5*30*/);
int tlfea_t10_retrieve_detj(tlfea_t10_t h, double *detJ /*E*5*/);
int tlfea_t10_retrieve_connectivity(tlfea_t10_t h, int *conn_colmajor /*E*10*/);
int tlfea_t10_retrieve_constraint_data(tlfea_t10_t h, double *c /*n_constraint*/);
int tlfea_t10_retrieve_constraint_jac_csr(tlfea_t10_t h, int *offsets /*nc+1*/, int *columns /*nc*/, double *values /*nc*/);
int tlfea_t10_retrieve_constraint_jact_csr(tlfea_t10_t h, int *offsets /*3N+1*/, int *columns /*nc*/, double *values /*nc*/);
int tlfea_t10_write_output_vtk(tlfea_t10_t h, const char *filename); /* FEAT10Data.cu:841-877 */

/* device pointers (FEAT10Data.cuh:648-666,781-783) */
const double *tlfea_t10_x12_device_ptr(tlfea_t10_t h);
const double *tlfea_t10_y12_device_ptr(tlfea_t10_t h);
const double *tlfea_t10_z12_device_ptr(tlfea_t10_t h);
double *tlfea_t10_external_force_device_ptr(tlfea_t10_t h);
double *tlfea_t10_constraint_device_ptr(tlfea_t10_t h);

/* ---- GPU_ANCF3243_Data / GPU_ANCF3443_Data -------------------------------------------------------------
 * The ANCF element types share the handle type and every `tlfea_t10_*` entry point above that is not
 * T10-specific (material setters, SetExternalForce, SetNodalFixed -- which takes COEFFICIENT indices for these
 * types, ANCF3243Data.cuh:778-808 --, CalcMassMatrix, CalcP, CalcInternalForce, CalcConstraintData, Retrieve*,
 * Destroy, and the whole SyncedNewtonSolver block below).  "Nodes" there means coefficient vectors
 * (n_coef = 4 * n_nodes; coefficient index = 4*node + slot, DOF = 3*coef + xyz).  Array sizes follow
 * tlfea_elem_dims(): gradients [E][Q][3][S], F/P [E][Q][9], connectivity [S][E] coefficient ids. */
int tlfea_ancf_create(int kind /*3243|3443*/, int n_nodes, int n_elements, tlfea_t10_t *out); /* ANCF3243Data.cuh:434-509, ANCF3443Data.cuh:445-520 */
/* Setup(L,W,H, mass rule, force rule, x12,y12,z12, connectivity) (ANCF3243Data.cuh:511-670, ANCF3443Data.cuh:522-670);
 * L,W,H per element; nqm/nq = {n_xi, n_eta, n_zeta}; conn_nodes E x nn (row-major unless conn_is_colmajor) */
int tlfea_ancf_setup(tlfea_t10_t h, const double *L, const double *W, const double *H, const double *gauss_xi_m,
                     const double *gauss_eta_m, const double *gauss_zeta_m, const double *weight_xi_m,
                     const double *weight_eta_m, const double *weight_zeta_m, const int *nqm,
                     const double *gauss_xi, const double *gauss_eta, const double *gauss_zeta,
                     const double *weight_xi, const double *weight_eta, const double *weight_zeta, const int *nq,
                     const double *x12, const double *y12, const double *z12, const int *conn_nodes,
                     int conn_is_colmajor);
int tlfea_ancf_calc_dsdu_pre(tlfea_t10_t h);
/* ANCF3243_B12_matrix / ANCF3443_B12_matrix (cpu_utils.cc:125-188, 211-420): the (B^T)^-1 matrix of one element,
 * column-major S x S (S = 8 | 16) -- the block layout of ANCF3243_B12_matrix_flat_per_element (cpu_utils.cc:190-209).
 * Host-only (no GPU touched); tlfea_ancf_setup computes the same blocks itself from L, W, H. */
int tlfea_ancf_b12_matrix(int kind /*3243|3443*/, double L, double W, double H, double *out_colmajor);
/* SetLinearConstraintsCSR (ANCF3243Data.cuh:810-940, ANCF3443Data.cuh same member): general linear constraints
 * c = J x - rhs, J in CSR over constraint rows, columns in the flattened DOF space (3*coef + component).  Accepted
 * on every element kind.  Must be called before BuildMassCSRPattern / CalcMassMatrix: the Hessian pattern includes
 * the coefficient pairs a row couples (SyncedNewton.cu:556-801).  Single-GPU path only. */
int tlfea_t10_set_linear_constraints_csr(tlfea_t10_t h, int n_rows, const int *offsets, const int *columns,
                                         const double *values, const double *rhs);
/* UpdateLinearConstraintRHS (ANCF3243Data.cuh / ANCF3443Data.cuh:977-997): new right-hand side of the CSR constraints,
 * J / J^T and the sparsity stay (prescribed motion: the airless-tire driver rotates its hub this way every step) */
int tlfea_t10_update_linear_constraint_rhs(tlfea_t10_t h, const double *rhs /*n_constraint*/, int n);
/* GetConstraintMode (ANCF3243Data.cuh:436-441): 0 none, 1 kConstraintFixedCoefficients, 2 kConstraintLinearCSR */
int tlfea_t10_get_constraint_mode(tlfea_t10_t h);
/* nnz of J (sizes the buffers of tlfea_t10_retrieve_constraint_jac_csr / _jact_csr) */
int tlfea_t10_constraint_jac_nnz(tlfea_t10_t h); /* CalcDsDuPre  ANCF3243Data.cu:290-300, ANCF3443Data.cu:256-266 */
int tlfea_elem_dims(tlfea_t10_t h, int *S /*shape functions*/, int *Q /*force quadrature points*/);

/* Stress and energy recovery of ANCF beam and shell meshes (no reference counterpart; DESIGN 3f').  The semantics are those
 * of tlfea_t10_calc_stress above with these differences: the handle is an ANCF one (a T10 handle is refused); d_vel / vel
 * have 3 * n_coef entries; point stresses are E * Q * 6 over the force-quadrature points (Q = 12 | 48, tlfea_elem_dims);
 * element values are means weighted by the reference volume (weights x det J of the element's L, W, H); "nodal" means per
 * MESH node (n_nodes = n_coef / 4), the V_e-weighted mean of the incident elements' means in ascending element order, von
 * Mises of that tensor; the kinetic energy 1/2 v.Mv runs over all coefficient DOFs (needs CalcMassMatrix).  Callable any
 * time after CalcDsDuPre; changes nothing a solver reads; every output is bitwise reproducible. */
int tlfea_ancf_calc_stress(tlfea_t10_t h, const double *d_vel /* device, 3*n_coef, or NULL */, int want_points);
int tlfea_ancf_calc_stress_host(tlfea_t10_t h, const double *vel /* host, 3*n_coef, or NULL */, int want_points);
int tlfea_ancf_retrieve_point_stress(tlfea_t10_t h, double *sigma /*E*Q*6*/);
int tlfea_ancf_retrieve_element_stress(tlfea_t10_t h, double *sigma /*E*6*/, double *von_mises /*E*/, double *psi /*E*/,
                                       double *J /*E*/, double *vol /*E*/); /* any may be NULL */
int tlfea_ancf_retrieve_nodal_stress(tlfea_t10_t h, double *sigma /*n_nodes*6*/, double *von_mises /*n_nodes*/); /* either may be NULL */
int tlfea_ancf_get_energies(tlfea_t10_t h, double out[5]);
double *tlfea_ancf_nodal_stress_device_ptr(tlfea_t10_t h); /* n_nodes*7: sigma, von Mises per mesh node; NULL before calc_stress */
/* mean ms over reps launches of: the point and element kernel, the mesh-node gather, the totals (profiling hook) */
int tlfea_ancf_time_stress_kernels(tlfea_t10_t h, const double *d_vel, int want_points, int reps, double *out_ms3);

/* ---- SyncedNewtonSolver --------------------------------------------------------------------- */
int tlfea_newton_create(tlfea_t10_t data, int n_constraints, tlfea_newton_t *out); /* SyncedNewton.cuh:37-149 */
int tlfea_newton_destroy(tlfea_newton_t s);                                        /* dtor :151-204 */
int tlfea_newton_setup(tlfea_newton_t s);                                          /* Setup :231-245 */
int tlfea_newton_set_parameters(tlfea_newton_t s, const tlfea_newton_params *p);   /* SetParameters :206-229 */
int tlfea_newton_analyze_hessian_sparsity(tlfea_newton_t s);                       /* SyncedNewton.cu:546-907 */
int tlfea_newton_set_fixed_sparsity_pattern(tlfea_newton_t s, int fixed);          /* :351-353 */
int tlfea_newton_solve(tlfea_newton_t s);            /* Solve()/OneStepNewtonCuDSS  SyncedNewton.cu:909-1394 */
double *tlfea_newton_velocity_guess_device_ptr(tlfea_newton_t s);                  /* :341-343 */
/* compute_l2_norm_cublas (SyncedNewton.cu:536-544) on a device vector */
int tlfea_newton_l2_norm(tlfea_newton_t s, const double *d_vec, int n, double *out);

/* ---- engine extras (no reference counterpart; used by tests/bench/INTEGRATION) -------------- */
int tlfea_newton_set_linsolve_opts(tlfea_newton_t s, const tlfea_linsolve_opts *o);
/* what the auto rules resolved to for this mesh: polynomial degree (1 = block-Jacobi), matrix bits of its steps and
 * the precision of its work vectors (32 on the single-GPU low-precision path, else 64) */
int tlfea_newton_get_linsolve_info(tlfea_newton_t s, int *cheb_degree, int *cheb_bits, int *cheb_vector_bits);
/* preconditioner a solve would use now: 0 block-Jacobi, 1 Chebyshev polynomial, 2 p-multigrid */
int tlfea_newton_get_precond(tlfea_newton_t s);
/* how compute_hessian_assemble_csr (FEAT10DataFunc.cuh:513-791) + the CSR scatter (SyncedNewton.cu:214-341) run now:
 * 1 = tangent blocks into an element-major buffer + row-owner gather (two launches; the ANCF kinds, TLFEA_ASSEMBLE=kbuf,
 *     meshes whose row groups do not fit the fused forms),
 * 2 = fused row-owner tangent + assembly, general form (one launch, no block buffer; T10 with curved elements or
 *     Mooney-Rivlin, TLFEA_ASSEMBLE=general),
 * 3 = fused row-owner tangent + assembly, affine-element form (T10, straight-sided elements, St.Venant-Kirchhoff) */
int tlfea_newton_get_assembly_mode(tlfea_newton_t s);
/* the launch an assembly would issue now (test hook), out8 = mode as above | 1 rolled kernel, 0 unrolled (general form;
 * 1 elsewhere) | wavefronts per workgroup of the tangent-block launch (mode 1; 0 in the fused modes) | row groups G (mode
 * 1: node rows) | doubles of LDS accumulator of the largest group (mode 1: of the longest row) | dynamic LDS bytes of the
 * assembly launch | workgroups it launches | entries of the pass table (mode 1: 1).  Runs the sparsity analysis if needed. */
int tlfea_newton_get_assembly_form(tlfea_newton_t s, int *out8);
/* how grad L gets its inertia term now (test hook): 1 = the mass CSR product with gathered velocities inside grad_kernel
 * (the ANCF kinds, TLFEA_MASS=csr), 2 = element inertia rows written by the residual launch and summed by
 * grad_light_kernel (T10 default) */
int tlfea_newton_get_gradient_form(tlfea_newton_t s);
/* degree of the coarse-level polynomial of the p-multigrid cycle (grows with the coarse mesh); 0 without p-multigrid */
/* third level of the cycle (rigid-body-mode aggregates of the vertex level; opt-in, TLFEA_PMG_LEVELS=3): number of
 * aggregates (0: two levels), 3x3 blocks of H3 (2 nodes per aggregate: translation, rotation), polynomial degree there;
 * retrieve: aggregate of every vertex node, x_i - c_A (zero where rotations are off), usable-rotation flags, the
 * level-3 block CSR and H3 = P2^T Hc P2 in the DOF-level layout of the other levels */
int tlfea_newton_pmg3_sizes(tlfea_newton_t s, int *n_aggregates, int *nnz_blocks, int *degree);
int tlfea_newton_pmg3_retrieve(tlfea_newton_t s, int *agg, double *rvec, int *active, int *off3, int *cols3, double *H3);
int tlfea_newton_pmg_coarse_degree(tlfea_newton_t s);
/* p-multigrid test hooks: coarse sizes; parent map [N] x 2, coarse block-CSR pattern and Hc = P^T H P of the current H
 * (9 nnz values in the DOF-level layout of H: node row -> [d][k][e]) */
int tlfea_newton_pmg_sizes(tlfea_newton_t s, int *n_coarse, int *nnz_coarse_blocks);
int tlfea_newton_pmg_retrieve(tlfea_newton_t s, int *par0, int *par1, int *c_off, int *c_cols, double *Hc);
/* Hc as the last preconditioner set-up (a solve or tlfea_newton_apply_preconditioner) left it on the device, nothing is
 * recomputed: the 9 nnz values, and in *form the kernel that summed them -- 1 the gather over the contribution lists
 * (ANCF), 2 the row kernel alone, 3 the row kernel fused with the streamed build of R, 4 the same fused pass on the image
 * rows of R assembled from the element records, with H itself left unassembled (TLFEA_SETUP_RECORDS).  Fails before the
 * first set-up and after tlfea_newton_pmg_retrieve / tlfea_newton_pmg3_retrieve, which sum Hc again, until the next set-up. */
int tlfea_newton_pmg_retrieve_built(tlfea_newton_t s, double *Hc, int *form);
/* Solve set-up from the element records (TLFEA_SETUP_RECORDS: 0 never, 1 wherever eligible, unset = eligible and at least
 * 400 000 node rows).  Where the CG's product, the fine smoother and the lambda_max product of a solve all run from the
 * element records and R is built in the pass that sums Hc (one GPU, uniform material, no term added to H after the fused
 * assembly), the Newton loop does not assemble H: it assembles the image rows of R, sum over the children of w H[child, :],
 * as rows of their own (the row function of a vertex is its linear hat function) and the fine block diagonal, and the set-up
 * sums Hc, D_c, sc_c and R from them.  Everything else that reads H (the read-backs, the hooks, the modal, direct and
 * adjoint solves, the CSR fall-backs of a solve) gets it assembled on demand from the point records while they are still
 * those of that assembly, and fails with a message that says so once they have moved (tlfea_newton_eval_gradient);
 * tlfea_newton_assemble_hessian always assembles.
 * out[0] = 1 if the last p-multigrid set-up ran on the image rows, 0 on the CSR H; out[1] = assemblies of H since the solver
 * was created; out[2] = 1 if the H on the device is the one of the last assembly. */
int tlfea_newton_get_setup_form(tlfea_newton_t s, long long out[3]);
/* Test hook: the image rows of the last such assembly, row I in H's row layout [d][len][3] at 9 r_off[I] (r_off: the row
 * offsets of tlfea_newton_pmg_restrict_op_retrieve); *len = 9 x blocks of R, image may be null (length only).  Fails when no
 * Newton iteration has taken the form yet. */
int tlfea_newton_get_setup_image(tlfea_newton_t s, double *image, long long *len);
/* Test hook: the fine level's 3x3 diagonal blocks [N][9], row-major, as the last preconditioner set-up read them off H or
 * the last assembly from the element records wrote them. */
int tlfea_newton_get_block_diagonal(tlfea_newton_t s, double *D);
/* Test hooks of the restricted fine operator R = S_c P^T S_f^-1 Hs, through which the V-cycle restricts the fine residual
 * (one GPU, first-kind smoother, 16- or 32-bit fine copy; TLFEA_PMG_RESTRICT_OP=0 keeps the fine residual pass).  They
 * copy back what the LAST preconditioner set-up (a solve or tlfea_newton_apply_preconditioner) left on the device and
 * rebuild nothing.  sizes: out6 = [0] 1 when that set-up built R, [1] vertex nodes Nc (rows of R), [2] 3x3 blocks of R,
 * [3] (child, fine block) contributions, [4] 3x3 blocks of H, [5] bits of the fine copy.  restrict_op_retrieve: R as it
 * is stored, node-level CSR off [Nc+1] / cols (ascending) and vals [blocks][9], each block row-major, fp32 widened to
 * double.  fine_copy_retrieve: the fine level's stored copy Hs = S_f H S_f in the node-block CSR of H (off [N+1], cols,
 * vals [blocks][9], fp16 / fp32 widened to double) and the scalings sc_f [3N], sc_c [3 Nc]. */
int tlfea_newton_pmg_restrict_op_sizes(tlfea_newton_t s, int *out6);
/* Test hook: launch geometry of the last NON-FINAL single-precision polynomial step on level 0 (fine), 1 (vertex) or 2
 * (third level): out7 = regime (0 last, 1 bandwidth, 2 latency, 3 one-round; -1 none yet), lanes per row, threads per
 * workgroup, blocks per lane issued up front, rows per group, grid, and the resident workgroups the occupancy query
 * answered for the instantiation launched (0 in the slot-capped regimes).  It is written where the host issues the launch:
 * when the CG iteration runs as a captured graph, that is at capture, and replays of the graph leave it as it is.
 * TLFEA_C32_REGIME=1|2|3|4 forces a regime (4: one-round with half the lanes); a forced one-round regime that does not
 * fit the device falls back to the automatic choice. */
int tlfea_newton_get_c32_geometry(tlfea_newton_t s, int level, int *out7);
/* Test hooks of the engine's own sparse direct solve (lin.method = 1, native backend), valid once a direct solve has
 * built its plan.  get_direct_info: out22 = plan facts [0] fronts, [1] levels, [2] top_depth (-1: every batch a whole
 * level; >= 0: fronts down to that depth one by one with a stack of update matrices), [3] doubles of the factor,
 * [4..7] doubles of the level buffers 0 / 1, the WORK buffer and the STACK, [8] largest front (DOF rows), [9] most own
 * columns of a front, [10] fronts without own columns, [11] nodes; then the kernel launches of the LAST factorisation +
 * solve, counted on the host next to each launch: [12] panel, [13] update inside a super-panel, [14] trailing update in
 * 64-tiles, [15] trailing update in 128-tiles, [16] extend-add, [17] stack push, [18] levels solved one workgroup per
 * front, [19] levels solved step by step, [20] forward steps, [21] backward steps.  get_direct_fronts: the elimination
 * order (new -> old node, [nodes]) and per front (children before parents) c0, c1 (own nodes: new positions [c0, c1)),
 * depth, parent, node rows, child 0, child 1 ([7 fronts]; -1: none).  The switches that steer the plan and the launches: TLFEA_DIRECT_LEAF,
 * _TOP_DEPTH, _MAX_NNZ, _SUPER, _WIDE_TILES, _ONE_WG_ROWS (DESIGN, "Sparse direct solve"). */
int tlfea_newton_get_direct_info(tlfea_newton_t s, long long *out22);
int tlfea_newton_get_direct_fronts(tlfea_newton_t s, int *order, int *fronts7);
int tlfea_newton_pmg_restrict_op_retrieve(tlfea_newton_t s, int *off, int *cols, double *vals);
int tlfea_newton_pmg_fine_copy_retrieve(tlfea_newton_t s, int *off, int *cols, double *vals, double *sc_f, double *sc_c);
/* Test hook of the fine level's low-precision copy.  A set-up that can still choose the fine smoother from the element
 * records does not convert it; fine_copy_retrieve, tlfea_newton_time_kernels and every pass that streams the copy convert
 * on demand from the H on the device and the scaling of the last set-up.  out3 = [0] bits of the copy allocated (0: none),
 * [1] 1 when the copy is that of the last set-up's H, [2] fine-level conversions since the solver was created. */
int tlfea_newton_get_fine_copy_state(tlfea_newton_t s, int *out3);
int tlfea_newton_hessian_nnz(tlfea_newton_t s, int *nnz);
/* H in the reference's DOF-level CSR (SyncedNewton.cu:163-205): rows 3N, sorted columns */
int tlfea_newton_retrieve_hessian_csr(tlfea_newton_t s, int *row_offsets, int *col_indices, double *values);
/* One residual evaluation at the current state: compute_p + internal force + constraints + grad L
 * (SyncedNewton.cu:1046-1065). Returns ||g||. */
int tlfea_newton_eval_gradient(tlfea_newton_t s, double *norm_g);
/* One Hessian assembly at the current state (SyncedNewton.cu:1080-1099). */
int tlfea_newton_assemble_hessian(tlfea_newton_t s);
/* Solve H x = b for host vectors (b,x length 3N) with the current H; iterations returned. */
int tlfea_newton_linear_solve(tlfea_newton_t s, const double *b, double *x, int *iters, double *rel_res);
/* mean duration (ms) of the hot kernels over `reps` back-to-back launches each (hipEvent pair per kernel on the
 * launch stream): [0] residual, [1] tangent blocks (0 in assembly mode 2), [2] row assembly (mode 2: the fused
 * tangent + assembly launch), [3] CG SpMV (fp64), [4] fine-level polynomial /
 * smoother step, [5] coarse-level polynomial step of the p-multigrid cycle, [6] the same kernel averaged over the
 * launch pattern of one V-cycle (3 fine + kc-1 coarse launches; [5], [6] are 0 without p-multigrid).  State of the
 * Newton iteration is unchanged (only linear-solver work vectors are touched). */
int tlfea_newton_time_kernels(tlfea_newton_t s, int reps, double *out_ms7);
/* y = H x with the current H, host vectors of 3N (partition-boundary rows summed over ranks). */
int tlfea_newton_apply_hessian(tlfea_newton_t s, const double *x, double *y);
/* ---- modal analysis (no reference counterpart) ---------------------------------------
 * The n_modes lowest pairs of  K phi = omega^2 M phi  on the free DOFs, K the tangent stiffness at the positions the data
 * object holds now (contact stiffness of rigid / field obstacles and the penalty of general linear constraints included;
 * pinned coefficients eliminated exactly), by LOBPCG on the shifted pencil A = K + shift M with the Newton solver's own
 * preconditioner.  shift (rad^2/s^2) must be positive -- it makes a free body's pencil definite -- and should be at or
 * below the lowest omega^2 of interest: any value gives the same modes, only the iteration count changes.
 * block_extra < 0 = auto (half of n_modes, at least 2).  Refused (tlfea_last_error says why): damping set, an obstacle with friction, a partitioned
 * mesh, lin.method = 1, n_modes < 1, n_modes + block_extra > 32, 3 x that above the free DOFs, no mass matrix.  The solver
 * is left as it was: time step, positions, velocities, multipliers, warm-start state; H is re-assembled. */
typedef struct {
  int n_modes, block_extra;
  double shift, tol; /* column i converged: ||K phi - omega^2 M phi|| <= tol (omega^2 + shift) ||M phi|| */
  int max_iter;
  unsigned seed;     /* of the deterministic start block */
} tlfea_modal_opts;
/* omega2 [n_modes] ascending; modes [n_modes][3N] M-normalised (may be NULL); resid [n_modes] the relative residuals of
 * the test above; info [4]: iterations, converged modes, block size, preconditioner (0 block-Jacobi, 1 polynomial,
 * 2 p-multigrid).  Returns an error, the outputs filled with what it has, when fewer than n_modes converge in max_iter. */
int tlfea_newton_modal_solve(tlfea_newton_t s, const tlfea_modal_opts *opts, double *omega2, double *modes, double *resid,
                             int *info);
/* test hooks: Y = H X (which 0) or (M (x) I3) X (which 1) with the current H for a host block [3N][m], m <= 32, pinned
 * rows zeroed when apply_mask; G [p][q] = X^T Y for host blocks [3N][p], [3N][q], p, q <= 96 */
int tlfea_newton_modal_apply_block(tlfea_newton_t s, int which, int m, const double *X, double *Y, int apply_mask);
int tlfea_newton_modal_gram(tlfea_newton_t s, int p, int q, const double *X, const double *Y, double *G);
/* mean ms of one block product Y = H X with m columns over `reps` launches (hipEvents; tools/modal_timing.py) */
int tlfea_newton_modal_time_spmm(tlfea_newton_t s, int m, int reps, double *ms_out);
/* ---- adjoint sensitivities of the implicit step (no reference counterpart) ---------------
 * One tlfea_newton_solve with max_outer = 1 finds v with g(v) = 0, x = x_prev + h v, then lambda_new = lambda + rho (J x - t)
 * and v_prev_new = v.  Given the cotangents x_bar, v_bar [3N] and lam_bar [n_constraints] of the outputs x, v, lambda_new
 * (NULL = zero), the adjoint step solves  H w = v_bar + h (x_bar + rho J^T lam_bar)  with the H of the current positions
 * and the solver's own tlfea_linsolve_opts (iterative or method = 1) and returns the cotangents of the step's inputs:
 *   f_ext_bar [3N] = w, v_prev_bar [3N] = M w / h, x_prev_bar [3N], lam_in_bar and t_bar [n_constraints] (t: the targets of
 *   fixed nodes, in the order 3 slot + component, or the right-hand side of the CSR rows), a_bar [3] (body acceleration),
 *   per_material [n_mat][P + 1] and per_element [E][P + 1]: the natural stiffness parameters of the model -- SVK
 *   (lambda, mu), P = 2; Mooney-Rivlin (mu10, mu01, kappa), P = 3 -- then the density.  n_mat = 1 without a table.
 * Any output may be NULL.  v_prev (NULL = the v_prev the last tlfea_newton_solve started from, which the solver keeps)
 * enters the density slot only.  All pointers are host pointers in tlfea_newton_adjoint_step and device pointers in
 * tlfea_newton_adjoint_step_device (a_bar and per_material included).  info[0] = iterations of the solve, rel_res its
 * ||r|| / ||b||.  The state must be that of a step just solved: positions, v; the call leaves x, v, v_prev, lambda and
 * the warm-start state of the linear solver as they were and re-assembles H.
 * Refused (tlfea_last_error says why): an ANCF handle, damping set (uniform or in a table entry), an obstacle with
 * friction, a follower pressure, a partitioned mesh, no mass matrix, and a last tlfea_newton_solve that ran more than one
 * outer iteration, failed, or left its Newton loop without meeting inner_atol / inner_rtol. */
typedef struct {
  const double *x_bar, *v_bar, *lam_bar, *v_prev;
} tlfea_adjoint_in;
typedef struct {
  double *f_ext_bar, *v_prev_bar, *x_prev_bar, *lam_in_bar, *t_bar, *a_bar, *per_material, *per_element;
} tlfea_adjoint_out;
int tlfea_newton_adjoint_step(tlfea_newton_t s, const tlfea_adjoint_in *in, const tlfea_adjoint_out *out, int *info,
                              double *rel_res);
int tlfea_newton_adjoint_step_device(tlfea_newton_t s, const tlfea_adjoint_in *in, const tlfea_adjoint_out *out, int *info,
                                     double *rel_res);
/* 0 when tlfea_newton_adjoint_step would accept the solver's state now, else the refusal (tlfea_last_error) */
int tlfea_newton_adjoint_ready(tlfea_newton_t s);
/* The element kernel and its reduction alone, at the current positions: host vectors w, u [3N] (u NULL: density slot 0),
 * per_element [E][P + 1] and per_material [n_mat][P + 1] as above (either may be NULL). */
int tlfea_t10_material_sensitivity(tlfea_t10_t h, const double *w, const double *u, double *per_element,
                                   double *per_material);
/* n_mat (1 without a table) and P + 1 of the object's model as it is set now */
int tlfea_t10_material_sensitivity_shape(tlfea_t10_t h, int *n_mat, int *slots);
/* mean ms over `reps` launches of out[0] the element kernel, [1] its reduction (hipEvents; tools/adjoint_timing.py) */
int tlfea_t10_time_sensitivity_kernels(tlfea_t10_t h, int reps, double *out_ms2);
/* ---- the same on ANCF-3243 beams and ANCF-3443 shells (DESIGN 3j'; no reference counterpart) ---------------------------
 * The step, tlfea_adjoint_in and tlfea_adjoint_out are those above with N = n_coef: every vector runs over the coefficient
 * vectors, positions and gradients alike.  What differs:
 *   - the body acceleration acts on the position coefficients (index % 4 == 0) only, so a_bar sums M w over those;
 *   - constraints are the fixed coefficients (constraint 3 slot + c = component c of coefficient fixed[slot]) or CSR rows;
 *   - the object has one material: per_material is [1][P + 1], per_element [E][P] (stiffness slots only: there is no
 *     per-element density, and the mass matrix is integrated with a rule of its own);
 *   - the density slot is -(M w) . u / rho0 with u = (v - v_prev)/h - a and rho0 the density the mass matrix was assembled
 *     with; a density <= 0 there is refused when per_material is wanted, and only then.
 * Refused (tlfea_last_error says why): a T10 handle, damping, an obstacle with friction, an ANCF follower pressure (dead
 * tractions and gravity are fine), a partitioned mesh, no CalcDsDuPre / BuildMassCSRPattern / CalcMassMatrix, and the
 * four states of the last tlfea_newton_solve that tlfea_newton_adjoint_step refuses.  The call leaves x, v, v_prev, lambda
 * and the warm-start state of the linear solver as they were and re-assembles H. */
int tlfea_newton_ancf_adjoint_step(tlfea_newton_t s, const tlfea_adjoint_in *in, const tlfea_adjoint_out *out, int *info,
                                   double *rel_res);
/* the same on device pointers (a_bar and per_material included) */
int tlfea_newton_ancf_adjoint_step_device(tlfea_newton_t s, const tlfea_adjoint_in *in, const tlfea_adjoint_out *out,
                                          int *info, double *rel_res);
/* 0 when tlfea_newton_ancf_adjoint_step would accept the solver's state now, else the refusal (tlfea_last_error) */
int tlfea_newton_ancf_adjoint_ready(tlfea_newton_t s);
/* The element kernel and the sums alone, at the current coefficients: host vectors w, u [3 n_coef] -> per_element [E][P]
 * and per_material [1][P + 1] (either may be NULL).  u NULL: density slot 0; u given: -(M w) . u / rho0, which needs the
 * mass matrix. */
int tlfea_ancf_material_sensitivity(tlfea_t10_t h, const double *w, const double *u, double *per_element,
                                    double *per_material);
/* n_mat (always 1) and P + 1 of the object's model as it is set now */
int tlfea_ancf_material_sensitivity_shape(tlfea_t10_t h, int *n_mat, int *slots);
/* mean ms over `reps` launches of out[0] the element kernel, [1] the sums of its P planes (hipEvents;
 * tools/ancf_adjoint_timing.py) */
int tlfea_ancf_time_sensitivity_kernels(tlfea_t10_t h, int reps, double *out_ms2);
/* ---- shape sensitivities of the implicit step (no reference counterpart) -----------------------------------
 * The same adjoint step with one more output: X_bar [3N] (interleaved like the other vectors; NULL = not wanted), the
 * cotangent of the reference coordinates of every node -- mid-edge nodes are coordinates of their own, a straight-sided
 * parametrisation by the vertices is the caller's chain rule.  It covers f_int, the inertia and the body acceleration
 * (both are M(X) times a vector); x_prev, the targets and f_ext do not depend on X.  tlfea_adjoint_in / tlfea_adjoint_out
 * are those of tlfea_newton_adjoint_step, which is this call with X_bar = NULL.  With X_bar wanted the call refuses, on top
 * of the list above, any rigid or field obstacle and any T10 face traction (their nodal weights are reference areas). */
int tlfea_newton_adjoint_step_shape(tlfea_newton_t s, const tlfea_adjoint_in *in, const tlfea_adjoint_out *out, double *X_bar,
                                    int *info, double *rel_res);
int tlfea_newton_adjoint_step_shape_device(tlfea_newton_t s, const tlfea_adjoint_in *in, const tlfea_adjoint_out *out,
                                           double *X_bar, int *info, double *rel_res);
/* The element kernel and its gather alone, at the current positions and reference geometry: host vectors w, u [3N] (u NULL:
 * no mass term; u needs an assembled mass matrix, whose densities the term uses) -> X_bar [3N]. */
int tlfea_t10_shape_sensitivity(tlfea_t10_t h, const double *w, const double *u, double *X_bar);
/* mean ms over `reps` launches of out[0] the element kernel, [1] its gather (hipEvents; tools/shape_timing.py) */
int tlfea_t10_time_shape_kernels(tlfea_t10_t h, int reps, double *out_ms2);
/* A new reference geometry X [n = number of nodes] for the same connectivity: grad N, det J and, if a mass matrix was
 * assembled, its values (same pattern, same densities) are recomputed; boundary-face geometry, traction vectors, the
 * constant load vector and obstacle surface weights follow.  Current positions, velocities, multipliers and targets are
 * left alone: the caller sets them.  The solver's sparsity, row groups and multigrid aggregates stay as analysed (they
 * order work and build a preconditioner; they do not enter the residual or H).  Refused: an ANCF handle; an element
 * with det J <= 0 at a quadrature point, which leaves the old geometry in place. */
int tlfea_t10_set_reference_positions(tlfea_t10_t h, const double *x, const double *y, const double *z, int n);
/* The same product from the matrix-free pair of the CG iteration (element records instead of the CSR values),
 * with the records of the last assembly.  Returns an error where that product is not eligible: anything but straight-sided
 * T10 elements with one St.Venant-Kirchhoff material on one GPU, general linear constraints, rigid obstacles, per-element
 * materials, or a residual evaluation since the last assembly. */
int tlfea_newton_apply_hessian_matfree(tlfea_newton_t s, const double *x, double *y);
/* which product the CG iterations of the last linear solve used: 0 = CSR kernel, 1 = matrix-free pair
 * (TLFEA_SPMV_MATFREE=0|1 forces it off / on where eligible; default: eligible and at least 150 000 nodes) */
int tlfea_newton_get_spmv_mode(tlfea_newton_t s);
/* fine smoother of the p-multigrid cycle the last preconditioner set-up chose: 0 = stream of the low-precision copy,
 * 1 = single-precision passes from the element records (DESIGN 3g'; TLFEA_PMG_FINE_MATFREE=0|1 forces it off / on where
 * eligible; default: eligible and at least 400 000 nodes) */
int tlfea_newton_get_fine_smoother(tlfea_newton_t s);
/* Test hook: one fine smoother pass of that form (res^ -= Hs d ; d' = c1 d + c2 (SDS)^-1 res^ ; z^ += zw d') with the
 * set-up a preceding tlfea_newton_apply_preconditioner left.  d, res, z: float [3N]; r: double [3N]; coef2 = (c1, c2); zw 0 =
 * no weight.  d_out always; last = 0: z_out, res_out (float [3N]); last = 1: z64_out = S z^' (double [3N]) and the 512 r.z
 * slots.  An error where the last set-up did not choose the form. */
int tlfea_newton_fine_smoother_pass(tlfea_newton_t s, const float *d, const float *res, const float *z, const double *r,
                                    const double *coef2, double zw, int last, float *d_out, float *z_out, float *res_out,
                                    double *z64_out, double *rz_slots);
/* the last lambda_max estimates: out[0] fine level, out[1] vertex level, out[2] third level (0 where there is none);
 * out[3] = 1 if the last fine estimate ran its products through the matrix-free pair (inside a solve whose CG iteration
 * does; TLFEA_LMAX_MATFREE=0 keeps the CSR product), else 0 */
int tlfea_newton_get_lambda_max(tlfea_newton_t s, double out[4]);
/* row form of the matrix-free pair once it has run: returns 1 where a wavefront of 64 elements sums its rows per node
 * before storing them (TLFEA_MATFREE_COMPACT, default 1), 0 for one row per (element, local node), -1 before the first
 * product.  rows = rows of the buffer, ratio = 10 E / rows (1 for the element form); either may be null. */
int tlfea_newton_get_matfree_rows(tlfea_newton_t s, long long *rows, double *ratio);
/* Test hook: the element records of the matrix-free passes of the assembled H.  which 0 / 1 = the element-major records
 * g [E][16] / F [E][5][10] in double; 2 / 3 = the packed lane-major g / F the kernels read (csrc/matfree_records.h): of the
 * fp64 product (single = 0, double; once a product has run) or of the fine smoother passes (single = 1, float; after a
 * preconditioner set-up that chose them).  len = values in that buffer, out may be null.  points = the stored points of
 * the packed F of that type (4 | 5: TLFEA_MATFREE_POINTS, or the default).  An error where those records do not exist. */
int tlfea_newton_get_matfree_records(tlfea_newton_t s, int single, int which, void *out, long long *len, int *points);
/* One full Newton iteration without the convergence test (gradient, assembly, solve, update):
 * the unit bench.py times.  iters = PCG iterations used. */
int tlfea_newton_iteration(tlfea_newton_t s, double *norm_g, int *iters);
int tlfea_newton_retrieve_gradient(tlfea_newton_t s, double *g /*3N*/);
int tlfea_newton_retrieve_velocity(tlfea_newton_t s, double *v /*3N*/);
int tlfea_newton_set_velocity(tlfea_newton_t s, const double *v /*3N*/, const double *v_prev /*3N or NULL*/);
int tlfea_newton_set_lambda(tlfea_newton_t s, const double *lam /*n_constraints multipliers*/);
int tlfea_newton_retrieve_lambda(tlfea_newton_t s, double *lam /*n_constraints*/);
/* stats of the last tlfea_newton_solve(): [0] outer iterations, [1] Newton solves, [2] last ||g||,
 * [3] last ||c||, [4] total PCG iterations, [5] device ms of the step (hipEvent) */
int tlfea_newton_get_stats(tlfea_newton_t s, double *stats6);
/* all-reduce calls the solver has issued since it was built (any exchange path); multi-GPU tests divide by CG iterations */
long tlfea_newton_collectives(tlfea_newton_t s);
/* number of multipliers the solver holds now (follows the data object's count at the start of every solve: an
 * UpdateNodalFixed with another size restarts them from zero) */
int tlfea_newton_n_constraints(tlfea_newton_t s);
/* linear solves since the last tlfea_newton_solve() / tlfea_newton_iteration() began: out4 = [0] ||r||/||b|| of the last
 * one, [1] 1 if it met rel_tol, [2] the worst ||r||/||b|| of them, [3] 1 if all of them met rel_tol */
int tlfea_newton_get_linsolve_status(tlfea_newton_t s, double *out4);
/* per-stage device time (ms, hipEvent pairs on the launch stream; profiling mode) and launch counts since
 * the last reset: [0] residual kernel, [1] gather+grad+norm, [2] tangent-block kernel, [3] row-assembly
 * kernel, [4] whole PCG solve, [5] update kernel, [6] SpMV kernel alone, [7] unused */
int tlfea_newton_get_stage_ms(tlfea_newton_t s, double *ms8, double *counts8, int reset);
/* start of an implicit step when driving Newton iterations by hand: x_prev <- x, v_prev <- v */
int tlfea_newton_begin_step(tlfea_newton_t s);
int tlfea_newton_set_verbose(tlfea_newton_t s, int verbose);
/* per-stage hipEvent timing for tlfea_newton_get_stage_ms (one host sync per stage; off by default) */
int tlfea_newton_set_profiling(tlfea_newton_t s, int on);

/* Multi-GPU hook: partition-boundary exchange (one process per GPU; elements are owned by one rank, nodes on
 * partition boundaries are replicated).  `iface_nodes[k]` (local node id) sits at `iface_slots[k]` of a GLOBAL
 * interface list of `n_global` nodes that is identical on every rank; `node_weight[i]` = 1/(number of ranks
 * holding node i).  The solver then calls `fn(user, d_buf, n)` -- in-place SUM over ranks of a device buffer
 * of n doubles -- exactly where the path needs it: once for the gradient (boundary DOFs), once for the
 * boundary diagonal blocks, and twice per CG iteration (boundary rows of H p fused with the p.Hp slots; the
 * r.z / r.r slots).  The Python host layer points fn at torch.distributed.all_reduce (RCCL over xGMI, or
 * gloo through a host staging copy).  f_ext must already be this rank's share (weight-scaled on replicated
 * nodes).  sync_before_callback=1 drains the stream before every call (needed unless fn enqueues on the
 * null stream, as torch's default stream does). */
typedef int (*tlfea_allreduce_fn)(void *user, double *d_buf, int n);
int tlfea_newton_set_interface(tlfea_newton_t s, const int *iface_nodes, const int *iface_slots, int n_local,
                               int n_global, const double *node_weight /*N*/, tlfea_allreduce_fn fn,
                               void *user, int sync_before_callback);
/* Built-in all-reduce for tlfea_newton_set_interface: RCCL called from C++ on the solver's launch stream -- no host
 * language in the loop, no host synchronisation (opt-in; the Python host layer's default goes through torch.distributed).
 * The RCCL library is resolved at run time (the copy already mapped into the process -- e.g. a PyTorch wheel's -- else
 * librccl.so from the loader path), so the engine carries no link-time dependency on it.
 *   rank 0: tlfea_rccl_unique_id(id) -> ship the 128 bytes to every rank -> tlfea_rccl_comm_create(id, rank, world, &comm)
 *   tlfea_newton_set_interface(..., tlfea_rccl_allreduce_fn(), comm, 0) ;  tlfea_rccl_comm_destroy(comm) at the end */
int tlfea_rccl_unique_id(char *id128);
int tlfea_rccl_comm_create(const char *id128, int rank, int world, void **comm_out);
int tlfea_rccl_comm_destroy(void *comm);
tlfea_allreduce_fn tlfea_rccl_allreduce_fn(void);
/* Owners of the replicated partition-boundary nodes: owned[N] = 1 where this rank owns the node (every node has exactly
 * one owner over all ranks; interior nodes: 1).  Makes the polynomial preconditioner rank-local (block-Jacobi over ranks:
 * no exchange inside the polynomial, one packed all-reduce per CG iteration for its result) instead of one exchange per
 * polynomial step.  Call after tlfea_newton_set_interface. */
int tlfea_newton_set_interface_owners(tlfea_newton_t s, const int *owned);

/* ---- Overlapping partition: owner-computes with ghost layers (the scalable multi-GPU path; the reference has no
 * counterpart -- it is a single-GPU code; SURVEY.md section 8e / north_star ask for it) ---------------------------------
 * Every node has ONE owning rank.  A rank's mesh (the data object it was built on) holds its owned nodes, `depth` layers
 * of ghost nodes (layer k = graph distance k from the owned set, nodes adjacent when they share an element) and every
 * element touching a node of layer < depth; local numbering: owned nodes first, then ghosts by increasing layer
 * (`node_layer` must be non-decreasing).  Rows of H, M and grad L of layers < depth are then complete on the rank:
 * nothing is summed over ranks.  The solver instead REFRESHES ghost values from their owners, neighbour to neighbour
 * (payload independent of the number of ranks), only where a step needs them: one nodal vector per CG iteration on the
 * fine level, the coarse polynomial's vectors once per `depth` steps (the overlap is computed redundantly in between),
 * the Newton update once per iteration, the diagonal blocks once per solve; dot products weigh owned DOFs 1 and ghosts 0
 * and are summed with `allreduce` (two fixed-size calls per CG iteration).  f_ext, fixed nodes and velocities are given
 * in full on every node the rank holds (no 1/multiplicity shares).
 * Lists: for peer k (`peers[k]`), send_nodes[send_off[k] .. send_off[k+1]) = my owned nodes that peer holds as ghosts,
 * ordered by (layer ON THE PEER = send_layer, global id); recv_nodes[...] = my ghosts owned by that peer ordered by
 * (own layer, global id) -- the peer's send list in the same order, so 'layers <= D' is a prefix on both sides.
 * exchange(user, d_send, d_recv, n_peers, peers, send_off, recv_off): for every peer k send bytes
 * [send_off[k], send_off[k+1]) of d_send to it and receive bytes [recv_off[k], recv_off[k+1]) of d_recv from it (device
 * buffers; empty ranges are skipped on both sides).  sync_before_callback as in tlfea_newton_set_interface. */
typedef int (*tlfea_halo_exchange_fn)(void *user, const void *d_send, void *d_recv, int n_peers, const int *peers,
                                      const long long *send_off, const long long *recv_off);
typedef struct {
  int n_peers;
  const int *peers;
  const int *send_off, *send_nodes, *send_layer;
  const int *recv_off, *recv_nodes;
  int rank, world; /* this rank and the number of ranks (world <= 0: unknown -- the replicated third multigrid level, which
                      gathers a few numbers per rank through the all-reduce, is then left out) */
} tlfea_halo_lists;
int tlfea_newton_set_halo(tlfea_newton_t s, const int *node_layer /*N*/, int depth, const tlfea_halo_lists *lists,
                          tlfea_allreduce_fn allreduce, tlfea_halo_exchange_fn exchange, void *user,
                          int sync_before_callback);
/* Built-in exchange on a communicator of tlfea_rccl_comm_create: one ncclGroup of ncclSend / ncclRecv pairs per refresh,
 * ncclAllReduce for the dot-product slots, all enqueued from C++ on the solver's launch stream, so the whole CG
 * iteration -- collectives included -- is captured in the solver's hipGraphs.  user = the communicator. */
tlfea_halo_exchange_fn tlfea_rccl_halo_exchange_fn(void);
/* Known-answer check of a fresh communicator (an all-reduce and a ring send/recv with values a rank can verify) under a
 * watchdog: returns 0 when every rank saw the right answers; on a wrong answer or when the collectives have not
 * completed after timeout_s seconds it prints the reason to stderr and terminates the PROCESS with exit code 97 (a
 * collective that never completes cannot be abandoned safely) -- the launcher sees a failed rank instead of a hang. */
int tlfea_rccl_self_check(void *comm, int rank, int world, double timeout_s);
/* tlfea_rccl_comm_create under the same watchdog (ncclCommInitRank blocks until every rank has joined). */
int tlfea_rccl_comm_create_timeout(const char *id128, int rank, int world, double timeout_s, void **comm_out);
/* Communication since the solver was built.  out8: [0] ghost refreshes (neighbour exchanges), [1] all-reduces,
 * [2] bytes sent in refreshes, [3] bytes all-reduced, [4] ms in exchanges + all-reduces measured with hipEvents on the
 * launch stream (only while tlfea_newton_set_profiling is on), [5] CG iterations, [6] / [7] the refreshes / all-reduces
 * issued INSIDE CG iterations (the per-iteration budget; the rest is per-solve set-up: diagonal blocks, lambda_max
 * estimates, the Newton update). */
int tlfea_newton_get_comm_stats(tlfea_newton_t s, double *out8);
/* Shape of the p-multigrid cycle a solve would run now (after the first solve or tlfea_newton_pmg_sizes): out6 = levels
 * (0: polynomial preconditioner), fine smoother terms, vertex-level smoother terms (three levels), vertex-level polynomial
 * degree (two levels), level-3 polynomial degree, level-3 nodes. */
int tlfea_newton_pmg_cycle_info(tlfea_newton_t s, int *out6);
/* Polynomial preconditioner in use (no reference counterpart: the reference calls cuDSS): out3 = degree, interval ratio
 * kappa (rounded), block size of the diagonal scaling of its operator -- 3 (per coefficient vector / node) or 12 (ANCF:
 * the four coefficient vectors of a node together, as a change of variables L^-1 H L^-T). */
int tlfea_newton_polynomial_info(tlfea_newton_t s, int *out3);
/* Test hooks: the CG preconditioner as an operator.  z = M^-1 r for host vectors of 3N with the current assembled H: the
 * warm state of the lambda_max estimates is reset, the preconditioner is set up as a solve sets it up (its cold lambda_max
 * estimate started from r; from a vector of ones when r is zero) and the function a CG iteration calls is applied once.
 * The _block form sets the operator up once, from the first vector, and applies it to m vectors R [m][3N] -> Z [m][3N]
 * (what a symmetry check needs: the operator depends on the start vector through lambda_max).  The warm state of the
 * linear solver is restored on return.  Refused on a partitioned mesh and with method = 1 (sparse direct). */
int tlfea_newton_apply_preconditioner(tlfea_newton_t s, const double *r, double *z);
int tlfea_newton_apply_preconditioner_block(tlfea_newton_t s, int m, const double *R, double *Z);
/* What the last set-up (a solve or the hook above) left on the device.  iout16: [0] preconditioner (0 block-Jacobi,
 * 1 polynomial, 2 p-multigrid), [1] levels (0, 2, 3), [2] polynomial degree, [3] fine smoother terms ks, [4..8] offsets of
 * the residual pair, the restart pair, the ks smoother weights, the vertex-level table and the level-3 polynomial in the
 * coefficient table, [9] vertex-level smoother terms ks2, [10] vertex-level polynomial degree kc, [11] level-3 degree k3,
 * [12] smoother kind (1 first-kind Chebyshev, 3 / 4 fourth kind), [13] doubles written to coef, [14] block size of the
 * polynomial's scaling (3 or 12), [15] matrix bits.  dout8: [0..2] lambda_max estimates (fine, vertex level, level 3) as
 * they stand now, [3] lam_safety, [4..6] the estimates of the last tlfea_newton_apply_preconditioner set-up.  coef: the
 * uploaded coefficient table copied back (pairs (c1, c2) per step), at most coef_cap doubles. */
int tlfea_newton_preconditioner_state(tlfea_newton_t s, int *iout16, double *dout8, double *coef, int coef_cap);
/* Test hook: the iterative solve of H x = b (host vector b [3N]) for exactly k iterations, 1 <= k <= 8 -- the solver's own
 * loop (set-up, start, first iteration launched eagerly, later ones replayed as graphs where graphs are on, residual
 * replacements where the mixed-precision iteration places them) with no convergence test before the last iteration --
 * and every iterate copied to the host on the way.  Record 0 is taken after the start (x = 0, r = b), record j after
 * iteration j - 1.
 *   vecs  [(k+1)][5][3N]: x, r, z, p, q.  p and q are those of the iteration just run, from the buffers that hold them (0 in
 *         record 0); after an iteration that ended with a residual replacement q is the replacement's H x.  With the
 *         block-Jacobi preconditioner z already belongs to the NEW r, with a polynomial one to the r the iteration
 *         started from.
 *   sums  [(k+1)][4]: the device's totals of the slot arrays r.z (even, odd iterations), p.q, r.r.
 *   slots [(k+1)][5][512]: the raw slot arrays (r.z even, r.z odd, p.q, r.r, b.b).
 *   form  [24], what ran: [0] fused direction update [1] lanes per row [2] non-temporal loads [3] tiled sweep [4] XCD
 *         eighths taken for this N and grid [5] grid of the product [6] graphs replayed [7] mixed-precision iteration
 *         [8] bit j: iteration j ended with a residual replacement [9] update kernel (0 block-Jacobi, 1 without z, 2 with
 *         the next polynomial's fp32 start vectors) [10] matrix-free product [11] polynomial degree [12] preconditioner
 *         (0 | 1 | 2) [13] matrix bits of the polynomial [14] 12 x 12 node blocks [15] grid of the update kernel [16..18]
 *         lanes, grid and XCD eighths of a residual replacement's fp64 product [19] TLFEA_XCD_ROWS mode.
 * The warm state is left as a solve of k iterations leaves it.  Refused on a partitioned mesh and with method = 1. */
int tlfea_newton_cg_trace(tlfea_newton_t s, const double *b, int k, double *vecs, double *sums, double *slots, int *form);

/* ---- SyncedAdamWNocoopSolver (SyncedAdamWNocoop.cuh:22-198, SyncedAdamWNocoop.cu:262-500) ------------------------
 * First-order ALM solver on the same velocity unknowns: per inner iteration one AdamW moment update, x = x_prev + dt v,
 * compute_p + internal force + constraints + grad L (the Newton solver's own residual path).  Single GPU. */
typedef struct tlfea_adamw_s *tlfea_adamw_t;
typedef struct { /* SyncedAdamWParams, field order of SyncedAdamW.cuh:27-34 */
  double lr, beta1, beta2, eps, weight_decay, lr_decay;
  double inner_tol, outer_tol, rho;
  int max_outer, max_inner;
  double time_step;
  int convergence_check_interval;
  double inner_rtol;
} tlfea_adamw_params;
int tlfea_adamw_create(tlfea_t10_t data, int n_constraints, tlfea_adamw_t *out); /* ctor SyncedAdamWNocoop.cuh:24-104 */
int tlfea_adamw_destroy(tlfea_adamw_t a);
int tlfea_adamw_setup(tlfea_adamw_t a);                                           /* Setup :180-198 */
int tlfea_adamw_set_parameters(tlfea_adamw_t a, const tlfea_adamw_params *p);     /* SetParameters :147-178 (also zeroes v, v_prev, lambda) */
int tlfea_adamw_solve(tlfea_adamw_t a);                                           /* Solve()/OneStepAdamWNocoop SyncedAdamWNocoop.cu:262-500 */
double *tlfea_adamw_velocity_guess_device_ptr(tlfea_adamw_t a);
int tlfea_adamw_retrieve_velocity(tlfea_adamw_t a, double *v);
int tlfea_adamw_retrieve_lambda(tlfea_adamw_t a, double *lam);
/* out6: outer iterations, inner iterations (total), last ||g||, last ||c||, inner-converged flag, device ms */
int tlfea_adamw_get_stats(tlfea_adamw_t a, double *out6);
/* 1: semantics of SyncedAdamWSolver, the cooperative-kernel sibling of the same solver (SyncedAdamW.cuh, SyncedAdamW.cu:
 * 96-345): inner-converged flag cleared once per Solve(), lam += rho dt c applied once (Nocoop: twice), outer loop stops
 * on ||c|| < outer_tol alone.  0 (default): SyncedAdamWNocoopSolver. */
int tlfea_adamw_set_cooperative_semantics(tlfea_adamw_t a, int on);
int tlfea_adamw_set_verbose(tlfea_adamw_t a, int v);

/* ---- SyncedNesterovSolver (SyncedNesterov.cuh:26-260, SyncedNesterov.cu:95-372) ---------------------------------
 * Accelerated-gradient ALM solver on the velocities (the reference's cooperative kernel as ordinary launches of the
 * same residual path).  Fixed-coefficient constraints, single GPU. */
typedef struct tlfea_nesterov_s *tlfea_nesterov_t;
typedef struct { /* SyncedNesterovParams (SyncedNesterov.cuh:26-30) */
  double alpha, rho, inner_tol, outer_tol;
  int max_outer, max_inner;
  double time_step;
} tlfea_nesterov_params;
int tlfea_nesterov_create(tlfea_t10_t data, int n_constraints, tlfea_nesterov_t *out);
int tlfea_nesterov_destroy(tlfea_nesterov_t a);
int tlfea_nesterov_setup(tlfea_nesterov_t a);                                          /* Setup :140-156 */
int tlfea_nesterov_set_parameters(tlfea_nesterov_t a, const tlfea_nesterov_params *p); /* SetParameters :118-138 */
int tlfea_nesterov_solve(tlfea_nesterov_t a);                                          /* Solve()/OneStepNesterov */
double *tlfea_nesterov_velocity_guess_device_ptr(tlfea_nesterov_t a);
int tlfea_nesterov_retrieve_velocity(tlfea_nesterov_t a, double *v);
int tlfea_nesterov_retrieve_lambda(tlfea_nesterov_t a, double *lam);
/* out6: outer iterations run, inner iterations (total), last ||g||, last ||c||, inner-converged flag, device ms */
int tlfea_nesterov_get_stats(tlfea_nesterov_t a, double *out6);
int tlfea_nesterov_set_verbose(tlfea_nesterov_t a, int v);


/* ---- SyncedVBDSolver (lib_src/solvers/SyncedVBD.cuh:13-21 params, :23-330 class; SyncedVBD.cu:163-400 node update,
 * :764-1135 Initialize*, :1475-1641 OneStepVBD) -- vertex block descent: ALM outer loop, inner loop of coloured
 * Gauss-Seidel sweeps of per-node 3x3 Newton updates on the velocities.  Pinned-node constraints only (the reference's
 * fixed map).  Call order of the reference drivers: create, Setup, SetParameters, InitializeColoring,
 * InitializeMassDiagBlocks, InitializeFixedMap, Solve per step (Solve runs the Initialize* it still needs). */
typedef struct tlfea_vbd_s *tlfea_vbd_t;
typedef struct { /* == SyncedVBDParams, same field order */
  double inner_tol, inner_rtol, outer_tol, rho;
  int max_outer, max_inner;
  double time_step, omega, hess_eps;
  int convergence_check_interval, color_group_size;
} tlfea_vbd_params;
int tlfea_vbd_create(tlfea_t10_t data, int n_constraints, tlfea_vbd_t *out);
int tlfea_vbd_destroy(tlfea_vbd_t a);
int tlfea_vbd_setup(tlfea_vbd_t a);                                         /* Setup  SyncedVBD.cuh:263-274 */
int tlfea_vbd_set_parameters(tlfea_vbd_t a, const tlfea_vbd_params *p);     /* SetParameters :228-261 */
int tlfea_vbd_initialize_coloring(tlfea_vbd_t a);                           /* SyncedVBD.cu:764-1028 */
int tlfea_vbd_initialize_mass_diag_blocks(tlfea_vbd_t a);                   /* :1030-1085 (runs CalcMassMatrix) */
int tlfea_vbd_initialize_fixed_map(tlfea_vbd_t a);                          /* :1087-1135 */
int tlfea_vbd_solve(tlfea_vbd_t a);                                         /* Solve()/OneStepVBD :1475-1641 */
/* colouring: sizes {n_colors, n_groups}; arrays colors[N], color_offsets[n_colors+1], color_nodes[N],
 * group_offsets[n_groups+1], group_colors[n_colors] (any pointer may be null) */
int tlfea_vbd_coloring_sizes(tlfea_vbd_t a, int *n_colors, int *n_groups);
int tlfea_vbd_retrieve_coloring(tlfea_vbd_t a, int *colors, int *color_offsets, int *color_nodes, int *group_offsets,
                                int *group_colors);
double *tlfea_vbd_velocity_guess_device_ptr(tlfea_vbd_t a);
int tlfea_vbd_retrieve_velocity(tlfea_vbd_t a, double *v);
int tlfea_vbd_retrieve_lambda(tlfea_vbd_t a, double *lam);
/* out6: outer iterations run, sweeps (total), last checked ||g||, last ||c||, 0, device ms */
int tlfea_vbd_get_stats(tlfea_vbd_t a, double *out6);
int tlfea_vbd_set_verbose(tlfea_vbd_t a, int v);

/* ---- HydroelasticPatchCollisionSystem (lib_src/collision/HydroelasticPatchCollisionSystem.h) ------------------------
 * Hydroelastic contact between tetrahedral meshes (T10 or T4): per-element AABB broadphase on a uniform grid,
 * one narrowphase work item per candidate pair (the plane where the two affine corner-pressure fields are equal,
 * clipped by both tets), and p_eq * area along the patch normal (optional normal damping and regularised friction)
 * distributed to the 8 corner nodes with the barycentric weights of the centroid.  The nodal sum is atomic-free and
 * bitwise reproducible: every node adds its contributions in patch order.  Pairs come out sorted by
 * (lower element id, higher element id).  Positions are read each step from a bound element object or a bound device
 * buffer; every launch runs on the default stream. */
typedef struct tlfea_contact_s *tlfea_contact_t;
/* ContactPatch (HydroelasticCollisionTypes / HydroelasticNarrowphase.cuh): tetA is on the mesh with the lower id; the
 * normal points from tet A into tet B; a patch with isValid == 0 or validOrientation == 0 applies no force */
typedef struct {
  double vertices[8][3];
  int count;
  double normal[3];
  double centroid[3];
  double area, g_A, g_B, p_equilibrium;
  int tetA, tetB;
  int isValid, validOrientation;
} tlfea_contact_patch;
/* ctor HydroelasticPatchCollisionSystem(nodes, elements, pressure, elementMeshIds, enableSelfCollision):
 * conn column-major n_elems x nodes_per_elem (10 or 4; the first 4 are the corners), pressure per node,
 * elem_mesh_ids per element (NULL: all elements on mesh 0).  Deviation: no neighbour set is built here -- with
 * self-collision the broadphase compares the node ids of a same-mesh candidate pair directly (equivalent filter) -- and
 * the node -> contribution lists of the force sum are rebuilt every step from that step's patches */
int tlfea_contact_create(int n_nodes, int n_elems, int nodes_per_elem, const int *conn_colmajor, const double *pressure,
                         const int *elem_mesh_ids, int self_collision, tlfea_contact_t *out);
int tlfea_contact_destroy(tlfea_contact_t c); /* dtor */
/* BindNodesDevicePtr: positions from the element object's own x / y / z buffers, read at every step (no copy) */
int tlfea_contact_bind_t10(tlfea_contact_t c, tlfea_t10_t data);
/* BindNodesDevicePtr(d_nodes): a device buffer [x..., y..., z...] of n_nodes nodes, read at every step */
int tlfea_contact_bind_nodes(tlfea_contact_t c, const double *d_colmajor, int n_nodes);
/* Step(CollisionSystemInput{d_vel}, CollisionSystemParams{damping, friction}): broadphase, narrowphase and the nodal
 * contact forces into the context's 3N buffer (xyz-interleaved); d_vel: device 3N interleaved velocities or NULL */
int tlfea_contact_step(tlfea_contact_t c, const double *d_vel, double damping, double friction);
/* engine extra: a host 3N force (gravity and the like) copied once and added by tlfea_contact_apply_to_t10 */
int tlfea_contact_set_base_force(tlfea_contact_t c, const double *f, int n);
/* engine extra: f_ext of the bound element object = base + contact force, on the device */
int tlfea_contact_apply_to_t10(tlfea_contact_t c);
/* GetExternalForcesDevicePtr */
double *tlfea_contact_force_device_ptr(tlfea_contact_t c);
/* GetNumContacts: candidate pairs of the last step */
int tlfea_contact_num_pairs(tlfea_contact_t c, int *n);
/* patches of the last step with isValid set */
int tlfea_contact_num_patches(tlfea_contact_t c, int *n);
/* RetrieveResults: pairs [n_pairs][2] (lower element id first), patches [n_pairs] in pair order, forces [3N] */
int tlfea_contact_retrieve_pairs(tlfea_contact_t c, int *pairs);
int tlfea_contact_retrieve_patches(tlfea_contact_t c, tlfea_contact_patch *patches);
int tlfea_contact_retrieve_force(tlfea_contact_t c, double *f);

#ifdef __cplusplus
}
#endif
#endif /* TLFEA_C_H */
