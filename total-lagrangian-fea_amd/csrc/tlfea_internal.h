// tlfea_internal.h -- device views and launch wrappers shared by the .hip translation units.
// gfx950 (MI355X) only.  Nothing here is part of the C-ABI (see include/tlfea_c.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "c32_geometry.h"
#include "row_sweep.h"
#include "mf_host.h"
#include "matfree_compact.h"
#include "matfree_records.h"

namespace tlfea {

// sets the message of tlfea_last_error(), prints it on stderr and returns 1 (tlfea_api.hip)
int api_fail(const std::string& msg);

constexpr int kNQ = 5;      // T10: Keast 5-point rule (quadrature_utils.h:134)
constexpr int kNN = 10;     // T10: nodes per element
constexpr int kMaxQ = 48;   // ANCF-3443 force rule 4x4x3 (quadrature_utils.h:22)
constexpr int kMaxS = 16;   // ANCF-3443 shape functions
constexpr int kWave = 64;   // CDNA wavefront

// element kinds: <S shape functions, Q force quadrature points>
enum ElemKind : int { kT10 = 0, kANCF3243 = 1, kANCF3443 = 2 };

enum MaterialModel : int { kSVK = 0, kMooneyRivlin = 1 }; // MaterialModel.cuh:14-17

// Material scalars travel as kernel arguments (SGPRs) -- the reference dereferences one device
// pointer per scalar per thread (FEAT10Data.cuh:825-829).
struct Material {
  int model;
  double lambda, mu;          // SVK
  double mu10, mu01, kappa;   // Mooney-Rivlin
  double eta, lamd;           // Kelvin-Voigt damping
  double rho0;
};

// Per-element materials (tlfea_t10_set_element_materials): one 64-byte record per element, expanded on the host from the
// material table and the element ids.  Slot kEmRhoM is the density the mass matrix was assembled with (the snapshot
// CalcMassMatrix takes), not the table's current one.  Only the kernels' per-element instantiations read it; the
// uniform ones keep taking Material by value.
constexpr int kEmRec = 8;
enum : int { kEmLambda = 0, kEmMu = 1, kEmEta = 2, kEmLamd = 3, kEmMu10 = 4, kEmMu01 = 5, kEmKappa = 6, kEmRhoM = 7 };
constexpr int kMaxMaterials = 256;  // table entries per object (tlfea_c.h)
struct MaterialPE {
  Material base;      // model; the scalars are unused
  const double* rec;  // [E][kEmRec]
};
__device__ __forceinline__ Material mat_at(const Material& m, int) { return m; }
__device__ __forceinline__ Material mat_at(const MaterialPE& m, int e) {
  const double2* r = reinterpret_cast<const double2*>(m.rec + (size_t)e * kEmRec);
  const double2 a = r[0], b = r[1], c = r[2], d = r[3];
  Material o;
  o.model = m.base.model;
  o.lambda = a.x; o.mu = a.y; o.eta = b.x; o.lamd = b.y;
  o.mu10 = c.x; o.mu01 = c.y; o.kappa = d.x; o.rho0 = d.y;
  return o;
}

// Device view of one mesh + state (all pointers are device pointers).  "N" counts coefficient vectors: nodes
// for T10, 4 per node (r, r_u, r_v, r_w) for the ANCF types.
struct ElemView {
  int E, N, Epad, S, Q;
  const int* conn;        // [S][E]   coefficient ids, column-major E x S (T10: the reference layout)
  const double* x;        // [N] current coordinates, SoA like the reference (d_h_x12/y12/z12)
  const double* y;
  const double* z;
  const double* gradN;    // [E][Q][3][S]  reference layout: wave-per-element kernels read contiguous runs
  const double* gradN_t;  // [Q][3][S][Epad] element-fastest copy: thread-per-element kernels coalesce
  const double* detJ;     // [E][Q]
  double qw[kMaxQ];       // combined quadrature weights
};

// T10 only: the inertia term M (v - v_prev) / h of grad L (SyncedNewton.cu:362-371) evaluated element by element in the
// residual launch (M = sum_e M_e with the rule of FEAT10Data.cu:206-278) instead of a CSR product with gathered
// velocities: Nq = shape functions at the 5 Keast points, rho = the density the mass matrix was assembled with.
struct MassTerm {
  const double* vprev;   // null: no mass term (mbuf is not written)
  double* mbuf;          // [10][Epad][6] per (node, element): force row | inertia row (replaces fbuf on this path)
  double rho_inv_h;      // rho0 / h
  double Nq[kNQ][kNN];
};

// node -> element incidence and the scatter map of the row-owner ("gather") assembly
struct Incidence {
  const int* n2e_off;   // [N+1]
  const int* n2e;       // [S*E]   e*S + local index, ascending e per node
  const int* n2e_pos;   // [S*E][S] position of column node conn(e,j) inside row i
  const int* off;       // [N+1]   node-level adjacency CSR (== mass CSR pattern)
  const int* cols;      // [nnz_coef] sorted per row
  const int* diagpos;   // [N]     position of i in row i
};

// Work lists of the fused tangent + assembly kernel (T10, SVK): a GROUP is a few node rows of H (3 CSR rows each) whose
// (row, incident element) instances are worked through in PASSES of up to 6; the resident wavefronts of an XCD walk
// that XCD's range of groups side by side (wave w takes groups w, w + W, w + 2W, ...).  Built once per mesh on the host
// (rowgroup_host.h): rows in Morton order of the reference coordinates, so that consecutive groups share elements.
struct RowGroups {
  int G;                  // groups
  int n_inst;             // S*E instances
  int acc_max;            // doubles of LDS accumulator the largest group needs
  const int* g_pass_off;  // [G+1] passes of group g
  const int4* pt;         // [P] pass: first instance | count + 8 first + 16 last of group + (rows << 8) | first row |
                          //          accumulator doubles of the group
  const int4* gr_info;    // [N] row: acc offset + (diagonal block position << 16) | off[row] | deg | node
  const int* gi_code;     // [S*E] element * S + local node, group order (ascending element inside a row)
  const int* gi_mb;       // [S*E] off[row] - acc offset / 3: mass value of an item's block = mval[gi_mb + acc / 3]
  const int* gi_pack;     // [S*E][S] per (instance, column node j): (acc offset of the block) | (3 deg << 16) |
                          //          bit 31: first contribution to the block (carries its M/h)
};

// Work lists of the affine-element form (assemble_affine_kernel; rowgroup_host.h build_row_groups4): passes of up to 16
// instances, 4 lanes per instance.
struct RowGroups4 {
  int G, n_inst, acc_max;
  const int* g_pass_off;  // [G+1]
  const int4* pt;         // [P] first instance | count (bits 0-4) + 32 first + 64 last + (rows << 8) | first row | acc doubles
  const int4* gr_info;    // [N] as RowGroups
  const int2* gi_head;    // [10 E] element * 10 + local row node | 3 deg
  const int2* gi_ent;     // [10 E][4] per (instance, vertex n): (acc offset / 3) of the blocks (n, p), p = 0..3, 16 bits each
};
// What the affine form knows about the mesh and the rule: straight-sided T10 elements have constant vertex gradients
// g_m = grad L_m and constant det J; the 5-point Keast rule has L = 1/4 at point q0 and L_m = 1/2 (others 1/6) at
// point qv[m].  gvec: [E][16] = g_0 | detJ | g_1 | - | g_2 | - | g_3 | -.
struct AffineView {
  const double* gvec;
  int q0, qv[4];
};

// ---- launch wrappers (defined in the .hip files) -------------------------------------------
void launch_dndu_pre(hipStream_t s, int E, int Epad, const int* conn, const double* x, const double* y,
                     const double* z, const double* qx, const double* qy, const double* qz,
                     double* gradN, double* gradN_t, double* detJ);
void launch_residual(hipStream_t s, const ElemView& m, const Material& mat, const double* v /*or null*/,
                     double* fbuf /*[E][30]*/, double* F, double* P, double* Fdot, double* Pvis,
                     double* Fq = nullptr /*[E][Q][9] row-major F per point, for the fused assembly*/,
                     const MassTerm* mt = nullptr /*T10: also write the per-element inertia rows*/,
                     double fq_h = 0.0 /*> 0: affine form, Fq holds [E][5][10] = F per point (centroid point first)*/,
                     int fq_slots = 0x43210 /*record slot of point q in bits 4q..4q+3 (the affine assembly's order)*/,
                     const double* emat = nullptr /*[E][kEmRec] per-element materials (T10), null = uniform mat*/);
// grad L without the mass CSR product (T10, inertia rows from the residual launch): 8 lanes per node
void launch_grad_light(hipStream_t s, int N, int Epad, const Incidence& inc, const double* fbuf, const double* mbuf,
                       const double* f_ext, const double* x, const double* y, const double* z, const double* xt,
                       const double* yt, const double* zt, const int* fixed_slot, const double* lam, const double* nw,
                       double h, double rho, double* f_int, double* cons, double* g);
// fused tangent + row assembly (T10, SVK): H rows straight from grad N and the F of the last residual launch
void launch_assemble_direct(hipStream_t s, const ElemView& m, const Material& mat, double h, const RowGroups& rg,
                            const double* Fq, const double* mval, const int* fixed_slot, const double* nw,
                            double penalty, double* Hval, const double* emat = nullptr);
// affine-element set-up: gvec from grad N / det J, and the largest relative deviation of the stored grad N / det J from
// the affine form (dev_max: one double on the device, zeroed by the caller)
void launch_affine_pre(hipStream_t s, const ElemView& m, const AffineView& av, double* gvec, double* dev_max);
// fused tangent + row assembly, affine elements: Fq16 = [E][5][10], F per point, centroid point first (last residual launch)
void launch_assemble_affine(hipStream_t s, const ElemView& m, const Material& mat, double h, const RowGroups4& rg,
                            const AffineView& av, const double* Fq16,
                            const double* cmass /*[10][16] sum_q w_q N_i N_j per (row node, vertex n, p); mid-edge columns halved*/,
                            double rho0 /*density of the assembled mass matrix, 0 = none (per-element: 1 = the
                                           records' kEmRhoM)*/, const int* fixed_slot,
                            const double* nw, double penalty, double* Hval, const double* emat = nullptr);
// Solve set-up from the element records (DESIGN 3g'): the unscaled image rows of R, (P^T H)[I, :] = sum over the children
// of w H[child, :], assembled as rows of their own -- the row function of coarse node I is the linear hat function of its
// vertex -- in H's row layout [d][len][3] at 9 r_off[I].  rg: build_row_groups4 on R's pattern with the (element, corner)
// instances; cmass4 [4][16]: cmass of the corner plus half that of its three mid-edge nodes (uniform material only).
void launch_assemble_image(hipStream_t s, const ElemView& m, const Material& mat, double h, const RowGroups4& rg,
                           const AffineView& av, const double* Fq16, const double* cmass4, double rho0, double* image);
// what the rows-out phase of the fine assembly adds to a pinned child's diagonal block, times the child's weight: one thread
// per (row, child) of R's child lists (ch_row: the row, ch_pos: position of the child's column in it); each entry has one writer
void launch_image_pinned(hipStream_t s, int n_ch, const int* ch, const float* ch_w, const int* ch_row, const int* ch_pos,
                         const int* r_off, const int* f_off, const int* fixed_slot, const double* nw, double penalty,
                         double* image);
template <typename R>
struct MatfreeCoefT;
struct ElemDiagMass {
  double c[kNN];  // rho / h x sum_q w_q N_a(q)^2
};
// the fine block diagonal D [N][9] from the packed fp64 records (np stored points): the element's ten diagonal blocks
// into dbuf [10][Epad][6], then the per-node sum in ascending element order + the pinned rows' penalty
void launch_records_diag(hipStream_t s, const ElemView& m, int np, const double* gp, const double* Fp,
                         const MatfreeCoefT<double>& mc, int N, const Incidence& inc, const int* fixed_slot, const double* nw,
                         double penalty, double* dbuf, double* D);
// Matrix-free product q = H p on affine elements (one material): the scalars of the assembled H, as
// launch_assemble_affine forms them, and the mass rule (N_j at the rule's points in the rule's order, its weights).
template <typename R>
struct MatfreeCoefT {
  R a, b, c1, cl;      // h lambda + lamd | h mu + eta | h mu | h lambda
  R w0, w1;            // weight of the centroid point | of the four outer points
  R rho_inv_h;         // density of the assembled mass matrix / h (0: none)
  R Nq[kNQ][kNN], mw[kNQ];
};
using MatfreeCoef = MatfreeCoefT<double>;
// Device lists of the compact row form (matfree_compact.h): a wavefront of 64 elements sums its rows per node first
struct MatfreeCompact {
  const int* row_off;           // [W + 1] first compact row of wavefront w
  const unsigned short* src;    // [W][640] LDS rows a * 64 + lane, grouped by compact row
  const unsigned short* desc;   // [W][640] start | (count - 1) << 10 per compact row of the wavefront
  const int* n2r_off;           // [N + 1]
  const int* n2r;               // [rows] compact rows of a node, ascending
};
// Packed copies in R of the records H was assembled from (matfree_records.h): Fq16 [E][5][10] -> Fp with np = 4 | 5
// stored points, gvec [E][16] -> gp; a null source is skipped
template <typename R>
void launch_matfree_pack(hipStream_t s, int E, int np, const double* Fq16, const double* gvec, R* Fp, R* gp);
// element rows of H p: ybuf [10][Epad][3], or with cp one row per (wavefront, node): ybuf [rows][3]; gp, Fp = the packed
// records with np = 4 | 5 stored points
void launch_tangent_apply_affine(hipStream_t s, const ElemView& m, int np, const double* gp, const double* Fp,
                                 const MatfreeCoef& mc, const double* p, double* ybuf, const MatfreeCompact* cp = nullptr);
// q = node-owner sum of the element rows (+ penalty x nw x p on pinned rows), p.q partials into the kNPart slots
void launch_matfree_gather(hipStream_t s, int N, int Epad, const Incidence& inc, const double* ybuf, const double* p,
                           const int* fixed_slot, const double* nw, double penalty, double* q, double* pq_part,
                           const MatfreeCompact* cp = nullptr);
// Fine smoother of the p-multigrid cycle from the element records, in single precision (DESIGN 3g').  One pass
//   res^ -= Hs d ; d' = c1 d + c2 (SDS)^-1 res^ ; z^ += zw d'      Hs = S H S
// is two launches.  The apply is tangent_apply_affine_kernel in float on float copies of the records (compact rows only),
// with the material scalars divided by m0 = max(|a|, |b|, |c1|, |cl|) and the direction x = (sc / sigma) d formed at the
// load (scn = float(sc / sigma), sigma^2 = mean(sc^2)): every factor is O(1) whatever the units.  The step sums a node's
// rows as matfree_gather_kernel does, adds the pinned-row term, multiplies by tau scn (tau = m0 sigma^2, formed on the
// device from ss = sum(sc^2): captured launch sequences stay valid when H moves; m0, the scalars and pen_m0 go to the
// kernels by value and are part of the CG graphs' key) and ends like cheb32_kernel.
struct FineMatfree {
  MatfreeCoefT<float> mc;       // scalars / m0
  double m0, pen_m0;            // m0 | h^2 rho / m0
  const float *gvec, *Fq;       // float copies of the records, packed (matfree_records.h)
  int np;                       // stored points of Fq: 4 | 5
  const float* scn;             // [3N] float(sc / sigma)
  const double* ss;             // device scalar sum(sc^2)
  double inv_n;                 // 1 / 3N
  float* ybuf;                  // [rows][3]
  const int* fixed_slot;
  const double* nw;
};
void launch_fine_matfree_apply(hipStream_t s, const ElemView& m, const FineMatfree& f, const float* d, const MatfreeCompact& cp);
void launch_fine_matfree_step(hipStream_t s, int N, const FineMatfree& f, const MatfreeCompact& cp, const float* Dinv_f,
                              const double* sc, const float* d_old, const double* coef, const double* zw, float* d_new,
                              const float* z, float* z_new, const float* res, float* res_new, const double* r, double* z_out,
                              double* rz_part, bool last);
// scn = float(sc / sigma) with sigma^2 = ss[0] * inv_n
void launch_fine_matfree_scale(hipStream_t s, int n, const double* sc, const double* ss, double inv_n, float* scn);
// What a launch of the assembly would use now -- the launchers' own arithmetic, not a restatement of it: dynamic LDS
// bytes, workgroups, and (general form) whether the rolled kernel runs.  The fused launchers call these themselves.
// They are not pure queries: the first call for a given LDS size also PREPARES the kernels as the launch needs them
// (hipFuncSetAttribute(MaxDynamicSharedMemorySize) above 64 KiB, the occupancy query behind the persistent grid) and
// caches the answers in function-local statics, exactly as the launchers did before the split.
struct AssemblyLaunchForm {
  size_t lds;
  int grid;
  int rolled;
};
AssemblyLaunchForm assemble_direct_form(const RowGroups& rg, const Material& mat, bool per_element);
AssemblyLaunchForm assemble_affine_form(const RowGroups4& rg, bool per_element);
AssemblyLaunchForm assemble_image_form(const RowGroups4& rg);  // launch_assemble_image
// the largest dynamic LDS any instantiation of a fused form takes for an accumulator of acc_max doubles (the material,
// hence the instantiation, may be switched between solves), and what assemble_rows_kernel takes for a longest row
size_t assemble_direct_lds_max(int acc_max);
size_t assemble_affine_lds_max(int acc_max);
size_t assemble_rows_lds(int maxdeg);
// LDS a workgroup can have on this device (hipDeviceAttributeMaxSharedMemoryPerBlock, queried once; MI355X: 163 840)
size_t device_lds_limit();
// wavefronts per workgroup of the tangent-block launch of the two-kernel path (TLFEA_TANGENT_WPB; 1 with per-element materials)
int tangent_blocks_wpb(bool per_element);
void launch_tangent_blocks(hipStream_t s, const ElemView& m, const Material& mat, double h,
                           double* Kbuf /*[E][55][9]*/, const double* emat = nullptr);
void launch_assemble_rows(hipStream_t s, int N, int S, int maxdeg, const Incidence& inc, const double* Kbuf,
                          const double* mval, double inv_h, const int* fixed_slot, const double* nw,
                          double penalty, double* Hval);
void launch_vbd_color(hipStream_t s, int lanes /*16|32|64 per node*/, const ElemView& m, const Material& mat,
                      const Incidence& inc, const int* nodes, int count, const double* mval, const double* f_ext, const int* fixed_slot, const double* xt,
                      const double* yt, const double* zt, const double* lam, double h, double rho, double omega,
                      double hess_eps, const double* v_prev, const double* xp, const double* yp, const double* zp,
                      double* v, double* x, double* y, double* z, const int* conn_rm /*[E][S]*/, double* xyz /*[N][3]*/,
                      const double* emat = nullptr, bool emat_damp = false /*some entry has eta or lamd != 0*/);
void launch_interleave_xyz(hipStream_t s, int N, const double* x, const double* y, const double* z, double* xyz);
void launch_mass_values(hipStream_t s, const ElemView& m, const Incidence& inc, const double* qx,
                        const double* qy, const double* qz, double rho0, double* mval,
                        const double* emat = nullptr /*per-element: density of slot kEmRhoM, rho0 unused*/);
void launch_grad(hipStream_t s, int N, const Incidence& inc, const double* fbuf, const double* mval,
                 const double* v, const double* vprev, const double* f_ext, const double* x,
                 const double* y, const double* z, const double* xt, const double* yt, const double* zt,
                 const int* fixed_slot, const double* lam, const double* nw, double h, double rho,
                 double* f_int, double* cons, double* g);
void launch_fint_gather(hipStream_t s, int N, const Incidence& inc, const double* fbuf, double* f_int);
// general linear constraints c = J x - rhs (CSR over constraint rows, columns = 3*coef + component)
void launch_lin_constraint(hipStream_t s, int nc, const int* joff, const int* jcol, const double* jval,
                           const double* rhs, const double* x, const double* y, const double* z, double* c);
void launch_lin_constraint_grad(hipStream_t s, int ndof, const int* jtoff, const int* jtcol, const double* jtval,
                                const double* lam, const double* c, double h, double rho, double* g);
void launch_lin_constraint_hessian(hipStream_t s, int ndof, const int* jtoff, const int* jtcol, const double* jtval,
                                   const int* joff, const int* jcol, const double* jval, const int* off,
                                   const int* cols, double f, double* H);
void launch_constraint(hipStream_t s, int n_fixed, const int* fixed_nodes, const double* x, const double* y,
                       const double* z, const double* xt, const double* yt, const double* zt, double* cons);

// vector / PCG kernels
constexpr int kNPart = 512; // partial sums per reduction (fixed -> run-to-run bitwise reproducible)
void launch_norm2(hipStream_t s, const double* a, const double* w /*weights or null*/, int n, double* part,
                  double* out /*device scalar: sum of squares*/);
void launch_extract_dinv(hipStream_t s, int N, const Incidence& inc, const double* Hval, double* Dinv);
void launch_pcg_init(hipStream_t s, int N, const double* b, const double* Dinv, const double* w, double* x,
                     double* r, double* z, double* rz_part, double* bb_part);
void launch_spmv_dir_dot(hipStream_t s, int N, const Incidence& inc, const double* Hval, const double* z,
                         const double* p_old, int first, const double* rz_part_old, const double* rz_part_new,
                         double* p_new, double* q, double* pq_part, bool fused, bool nt, const double* wown = nullptr);
// what a launch of the CG's product kernel on N rows is: instantiation (fused direction update, lanes per row,
// non-temporal loads) and geometry (tiled sweep, TLFEA_XCD_ROWS mode, XCD eighths taken -- row_sweep.h -- and grid)
struct SpmvForm {
  int fused = 0, lanes = 32, nt = 0, tiled = 1, xcd_mode = 1, xcd = 0, grid = 1;
};
SpmvForm spmv_form(int N, bool fused, bool nt, bool f32);
int slot_grid_256(int n);  // workgroups of the 256-thread update kernels over n items
void launch_pcg_direction(hipStream_t s, int n, const double* z, int first, const double* rz_part_old,
                          const double* rz_part_new, double* p);
void launch_pcg_update(hipStream_t s, int N, const double* Dinv, const double* w, const double* p, const double* q,
                       const double* rz_part_old, const double* pq_part, double* x, double* r, double* z,
                       double* rz_part_new, double* rr_part);
void launch_sum_parts(hipStream_t s, const double* part, double* out);
void launch_cheb_init(hipStream_t s, int N, const double* Dinv, const double* r, const double* sc,
                      const double* coef, double* d, double* z, double* res);
void launch_cheb_step(hipStream_t s, int N, const Incidence& inc, const double* Hval, const double* Dinv,
                      const double* d_old, const double* coef, double* d_new, double* z, double* res,
                      const double* r, const double* w, double* rz_part, bool last);
void launch_cheb_update(hipStream_t s, int N, const double* Dinv, const double* q, const double* d_old,
                        const double* coef, double* d_new, double* z, double* res, const double* r, const double* w,
                        const double* sc, double* rz_part, bool last);
// low-precision (fp16/fp32) scaled block-CSR copy of H for the polynomial preconditioner
void launch_lp_scale(hipStream_t s, int N, const double* D, const double* Dinv, double* sc, double* Dinv_s);
void launch_lp_convert(hipStream_t s, int N, const Incidence& inc, const double* Hval, const double* sc, const int* own,
                       const double* Dglob, void* B8, void* B1, int bits);
void launch_mask_scale(hipStream_t s, int N, const double* sc, const int* own, double* out);
// the polynomial in single precision (single-GPU path): fp32 vectors, fp16/fp32 matrix, fp32 accumulation
void launch_spmv_dir_dot_f32(hipStream_t s, int N, const Incidence& inc, const float* Hval32, const double* z,
                             const double* p_old, int first, const double* rz_part_old, const double* rz_part_new,
                             double* p_new, double* q, double* pq_part, bool fused, const double* wown = nullptr);
void launch_residual_replace_init32(hipStream_t s, int N, const double* b, const double* q, double* r, double* rr_part,
                                    const float* Dinv_f, const double* sc, const double* coef, float* d, float* z,
                                    float* res, const double* wown = nullptr);
// overlapping partition: ghost refresh messages (nvec fields of dim values per node, interleaved per node)
void launch_halo_pack(hipStream_t s, int n, const int* idx, int dim, int nvec, const double* a, const double* b,
                      const double* c, double* msg);
void launch_halo_unpack(hipStream_t s, int n, const int* idx, int dim, int nvec, const double* msg, double* a, double* b,
                        double* c);
void launch_halo_pack(hipStream_t s, int n, const int* idx, int dim, int nvec, const float* a, const float* b,
                      const float* c, float* msg);
void launch_halo_unpack(hipStream_t s, int n, const int* idx, int dim, int nvec, const float* msg, float* a, float* b,
                        float* c);
void launch_to_float(hipStream_t s, size_t n, const double* a, float* b);
void launch_cheb32_init(hipStream_t s, int N, const float* Dinv_f, const double* r, const double* sc,
                        const double* coef, float* d, float* z, float* res, int row0 = 0);
// Partition-boundary rows of the single-precision polynomial on the multi-GPU path: their Hs d is the SUM over ranks of
// the ranks' partial rows (launch_spmv32_rows -> all-reduce), handed to the fused step through bsum; w = 1/multiplicity
// of a DOF in the r.z partials of the last step.
struct C32Bnd {
  const int* bslot = nullptr;    // [N] slot of a boundary node in the exchange buffer, -1 for interior nodes
  const double* bsum = nullptr;  // [3 slots] summed Hs d of the boundary rows
  const double* w = nullptr;     // [3N] weights of the r.z partials (last step), null = 1
  const double* zw = nullptr;    // device scalar: z^ += zw d' instead of z^ += d' (fourth-kind Chebyshev smoothers), null = 1
  int xcd = 0;                   // set by the launcher: XCD-aware row sweep (solver_kernels.hip, row_sweep)
};
void launch_cheb32(hipStream_t s, int N, int nnz_coef, const Incidence& inc, const void* B8, const void* B1, int bits,
                   const float* Dinv_f, const double* sc, const float* d_old, const double* coef, float* d_new,
                   const float* z, float* z_new, const float* res, float* res_new, const double* r, double* z_out,
                   double* rz_part, bool last, C32Bnd bnd = C32Bnd(), C32Geometry* chosen = nullptr /*out: the geometry launched*/);
// out[3 slot[k] + c] = (Hs d)_{rows[k], c} for a list of rows (this rank's part of the partition-boundary rows)
void launch_spmv32_rows(hipStream_t s, int n_rows, const int* rows, const int* slots, const Incidence& inc, const void* B8,
                        const void* B1, int bits, const float* d, double* out);
// restriction of the partition-boundary coarse rows only: out[3 slot[k] + c] = sum_children w res_f / sc_f (this rank's part)
void launch_pmg_restrict_rows(hipStream_t s, int n_rows, const int* rows, const int* slots, const int* child_off,
                              const int* child, const float* child_w, const float* res_f, const double* sc_f, double* out);
// two-level p-multigrid (T10): Galerkin coarse operator and grid transfers (pmg_host.h holds the integer set-up)
void launch_pmg_galerkin(hipStream_t s, int n_upper, const int* c_upper, const int* c_mirror, const int* c_off,
                         const int* cblk_row, const int* con_off, const int* con_base, const int* con_deg,
                         const float* con_w, const double* Hf, double* Hc);
void launch_pmg_restrict_init(hipStream_t s, int Nc, const int* child_off, const int* child, const float* child_w,
                              const float* res_f, const double* sc_f, const double* sc_c, const float* Dinv_c,
                              const double* coef_c, float* d_c, float* z_c, float* res_c, const int* bslot = nullptr,
                              const double* bsum = nullptr);
// third level: rigid-body-mode aggregation of the vertex level (pmg_host.h agg_build)
void launch_agg_galerkin(hipStream_t s, int n_pairs, const int* pair_A, const int* pair_pos, const int* pair_B,
                         const int* pcon_off, const int* pcon_base, const int* pcon_deg, const int* pcon_i,
                         const int* pcon_j, const double* rvec, const int* active, const int* off3, const double* Hc,
                         double* H3);
void launch_agg_restrict_init(hipStream_t s, int N3, const int* mem_off, const int* mem, const double* rvec,
                              const float* res2, const double* sc2, const double* sc3, const float* Dinv3,
                              const double* coef3, float* d3, float* z3, float* res3);
void launch_agg_restrict(hipStream_t s, int N3, const int* mem_off, const int* mem, const double* rvec, const float* res2,
                         const double* sc2, double* r3);
void launch_agg_init3(hipStream_t s, int N3, const double* r3, const double* sc3, const float* Dinv3, const double* coef3,
                      float* d3, float* z3, float* res3);
void launch_agg_prolong(hipStream_t s, int Nc, const int* agg, const double* rvec, const float* z3, const double* sc3,
                        const double* sc2, float* z2, float* d2);
void launch_pmg_prolong(hipStream_t s, int N, const int* par0, const int* par1, const float* z_c, const double* sc_c,
                        const double* sc_f, float* z_f, float* d_f, bool add_to_d = false);
// restricted fine operator R = S_c P^T S_f^-1 Hs (pmg_host.h pmg_restrict_op_build): build from the stored fine copy (once
// per solve), and the restriction  r^_c = S_c P^T S_f^-1 res_f - R d_f  fused with the coarse start vectors
void launch_pmg_rop_build_h(hipStream_t s, int Nc, const int* r_off, const int* r_cols, const int* con_off, const int* con_blk,
                            const unsigned char* con_ord, const int* ch_off, const int* ch, const float* ch_w, const int* f_off,
                            const double* Hval, const double* sc_f, const double* sc_c, void* R8, float* R1);
// The T10 vertex level's Hc = P^T H P, and with_R the same R, from an image of the R row (DESIGN 3g'): a wavefront per
// coarse row streams its children's rows of H into the image, sums the row's blocks of Hc (column >= row, mirrored) from
// it and, with_R, scales the image into the row of R with sc_c formed from the diagonal block just summed.  Rows of at
// most cap <= kRopStreamCap blocks keep the image in LDS; the n_long longer ones (long_rows, ascending) take the same
// code with the image in a slice of ws (ws_stride doubles each, ws_rows slices: that many rows a launch).
constexpr int kRopStreamCap = 128;  // blocks of the image: 9 KB per wavefront, 12 wavefronts per CU
struct PmgRows {
  // the row structure of R (pmg_host.h RopHost), the fine row offsets and H
  const int *r_off, *r_cols, *pos_off;
  const unsigned short* con_pos;
  const int *ch_off, *ch;
  const float* ch_w;
  const int* f_off;
  const double* Hval;
  // the combine (GalRowsHost) and the coarse pattern; D: the diagonal blocks [Nc][9] as well, null = not wanted
  const int *g_row, *g_off;
  const unsigned short* g_pos;
  const unsigned char* g_w;
  const int *c_off, *c_upper, *c_mirror, *cblk_row;
  double *Hc, *D;
  // with_R only: the fine scaling and R's values (8 + 1 floats per block)
  const double* sc_f;
  void* R8;
  float* R1;
};
void launch_pmg_galerkin_rows(hipStream_t s, int Nc, int cap, const PmgRows& a, bool with_R, const int* long_rows, int n_long,
                              size_t ws_stride, int ws_rows, double* ws);
void launch_pmg_rop_build(hipStream_t s, int Nc, const int* r_off, const int* con_off, const int* con_blk,
                          const unsigned char* con_ord, const int* ch_off, const int* ch, const float* ch_w, const void* B8,
                          const void* B1, int bits, const double* sc_f, const double* sc_c, void* R8, float* R1);
void launch_pmg_restrict_op_init(hipStream_t s, int Nc, int nnz_r, const int* child_off, const int* child,
                                 const float* child_w, const float* res_f, const float* d_f, const double* sc_f,
                                 const double* sc_c, const int* r_off, const int* r_cols, const void* R8, const float* R1,
                                 const float* Dinv_c, const double* coef_c, float* d_c, float* z_c, float* res_c);
// test hooks: a streamed copy (bits 16 or 32) widened to doubles, [nnz][9]
void launch_lp_widen(hipStream_t s, size_t nnz, const void* B8, const void* B1, int bits, double* out);
// mode 0: Chebyshev step, 1: last step (z back in the unscaled space + r.z slots in out), 2: out = Hs d_old
void launch_cheb_lp(hipStream_t s, int N, int nnz_coef, const Incidence& inc, const void* B8, const void* B1, int bits,
                    const double* Dinv_s, const double* sc, const double* d_old, const double* coef, double* d_new,
                    const double* z, double* z_new, const double* res, double* res_new, const double* r,
                    const double* w, double* out, int mode);
void launch_pcg_update_init32(hipStream_t s, int N, const double* p, const double* q, const double* rz_part_old,
                              const double* pq_part, double* x, double* r, double* rr_part, double* indefinite,
                              const float* Dinv_f, const double* sc, const double* coef, float* d, float* z,
                              float* res, const double* wown = nullptr);
void launch_pcg_update_noz(hipStream_t s, int N, const double* w, const double* p, const double* q,
                           const double* rz_part_old, const double* pq_part, double* x, double* r, double* rr_part,
                           double* indefinite);
void launch_apply_dinv(hipStream_t s, int N, const double* Dinv, const double* q, double* v);
// block-vector kernels of the modal solve (modal_kernels.hip): a block holds ld doubles per DOF row, the m
// columns of a DOF contiguous; fixed_slot (or null) zeroes the rows of pinned nodes at write-out
void launch_spmm_block(hipStream_t s, int N, int m, const int* off, const int* cols, const double* Hval, const double* X,
                       int ldx, double* Y, int ldy, const int* fixed_slot);
void launch_massmm_block(hipStream_t s, int N, int m, const int* off, const int* cols, const double* mval, const double* X,
                         int ldx, double* Y, int ldy, const int* fixed_slot);
size_t gram_slot_doubles(int n, int p, int q);  // doubles of the slot buffer a launch_gram of p x q over n rows needs
void launch_gram(hipStream_t s, int n, int p, int q, const double* X, int ldx, const double* Y, int ldy, double* slots,
                 double* G /*[p][q] = X^T Y*/);
void launch_block_combine(hipStream_t s, int n, int k, double* S, int ld, const double* C /*[k][nz]*/, int nz, int nz0,
                          int z0, int z1);
void launch_block_residual(hipStream_t s, int n, int m, const double* AX, const double* MX, int ld, const double* mu,
                           double* R, int ldr, double* slots, double* norms2 /*[m] |r|^2, [m] |Mx|^2*/);
void launch_block_get_col(hipStream_t s, int n, const double* B, int ld, int j, double* v);
void launch_block_set_col(hipStream_t s, int n, const double* v, const int* fixed_slot, double* B, int ld, int j);
void launch_block_hash(hipStream_t s, int n, int m, unsigned seed, const int* fixed_slot, double* B, int ld);
void launch_scale(hipStream_t s, int n, double a, double* v);
void launch_scale_inv_sqrt(hipStream_t s, int n, const double* sumsq, double* v);
void launch_newton_update(hipStream_t s, int N, const double* dv, double* v, const double* xp, const double* yp,
                          const double* zp, double h, double* x, double* y, double* z);
void launch_axpy_neg(hipStream_t s, int n, const double* g, double* r);
void launch_diff(hipStream_t s, int n, const double* a, const double* b, double* r);  // r = a - b
void launch_adamw_update_velocity(hipStream_t s, int n, const double* g, double beta1, double beta2, double eps,
                                  double weight_decay, double lr, double inv_1mb1t, double inv_1mb2t, double* m,
                                  double* va, double* v);
void launch_nesterov_lookahead(hipStream_t s, int n, double beta, const double* vk, const double* vkm1, double* v);
void launch_nesterov_step(hipStream_t s, int n, double alpha, const double* y, const double* g, double* vnext);
void launch_positions_from_prev(hipStream_t s, int N, const double* v, const double* xp, const double* yp,
                                const double* zp, double dt, double* x, double* y, double* z);
void launch_dual_update(hipStream_t s, int nc, const double* cons, double rho, double* lam);
void launch_pack(hipStream_t s, int n, int dim, const int* node, const int* slot, const double* src, double* buf);
void launch_unpack(hipStream_t s, int n, int dim, const int* node, const int* slot, const double* buf, double* dst);
void launch_extract_diag(hipStream_t s, int N, const Incidence& inc, const double* Hval, double* D);
void launch_invert_diag(hipStream_t s, int N, const double* D, double* Dinv);

// ANCF node-block (12 x 12) scaling of the polynomial's operator (solver_kernels.hip)
void launch_blk12_factor(hipStream_t s, int Np, const Incidence& inc, const double* Hval, double* Linv, float* Linv_f,
                         double* sc, double* Dinv_s, int* err);
void launch_blk12_apply(hipStream_t s, int Np, const float* Linv_f, bool transpose, const double* in, double* out);
void launch_lp_convert12(hipStream_t s, int N, const Incidence& inc, const double* Hval, const double* Linv, void* B8,
                         void* B1, int bits);

// ---- sparse direct solve (direct_kernels.hip on the plan of mf_host.h) ------------------------------------------------
struct MfFrontDev {  // a front as the kernels see it (DOF units)
  long long F_off, L_off, v_off, map_off, rows_off;
  long long cF_off;  // where its PARENT reads its update matrix (the front itself, or its compact copy on the stack) ...
  int m, k, c0, child0, child1;
  int c_ld, c_k0, pad;  // ... with this leading dimension and first row / column
};
struct MfDev {
  const MfFrontDev* fr;
  const int *lvl, *blvl, *map, *rows, *order;  // lvl: fronts by level (solve), blvl: fronts by batch (factorisation)
  const long long *hsrc, *hdst;
  const int *hsld, *hdld;
  double* L;
  double* F[4];  // front workspaces: level buffers (depth parity), WORK, STACK (mf_host.h, MfBatch)
  double *v, *y, *xp;
  int* err;
};
// Launches issued by the last launch_mf_factor / launch_mf_solve, counted on the host next to each launch
// (tlfea_newton_get_direct_info): which kernels a plan and the TLFEA_DIRECT_* switches actually reached.
struct MfTally {
  long long panel = 0, update_inner = 0, update_trailing = 0, update_wide = 0, extend_add = 0, push = 0;  // factorisation
  long long levels_one_wg = 0, levels_stepwise = 0, fwd_step = 0, bwd_step = 0;                           // solve
};
void launch_mf_factor(hipStream_t s, const MfPlan& P, const MfDev& D, const double* H, MfTally& tally);
void launch_mf_solve(hipStream_t s, const MfPlan& P, const MfDev& D, const double* b, double* x, MfTally& tally);

// Rigid analytic obstacles (tlfea_t10_set_obstacles): the list travels by value in the kernel arguments
// (16 x 120 bytes).  Every surface node owns its own entries of g, of its diagonal block of H and of the per-node
// buffers, so the launches need no atomics and are bitwise reproducible.
constexpr int kMaxObstacles = 16;
enum ObstacleKind : int { kHalfSpace = 0, kSphere = 1, kField = 2 };
// A field obstacle (tlfea_set_field_obstacles, DESIGN 3e''): nx x ny x nz signed-distance samples V[(iz ny + iy) nx + ix]
// at origin + spacing (ix, iy, iz) in the obstacle's frame, rot (row-major) frame -> world.  The descriptors and the
// samples live in device memory; the list entry carries the descriptor's address, its position in p and the rest of
// the contact parameters as an analytic obstacle does.
struct FieldDev {
  int nx, ny, nz;
  double origin[3], spacing, rot[9];
  const double* V;
};
struct ObstacleDev {
  int kind;
  double p[3], n[3], radius, vel[3], kappa, mu, eps_v;
  const FieldDev* fld;  // kField only
};
struct ObstacleList {
  int n;
  ObstacleDev o[kMaxObstacles];
  bool has_fields() const {  // host: which instantiation of the obstacle kernels a launch takes
    for (int j = 0; j < n; j++)
      if (o[j].kind == kField) return true;
    return false;
  }
};
// Per surface node k (node[k]): force f = -grad Phi (3), symmetric 3x3 block of the Hessian of Phi (xx yy zz xy xz yz),
// and per obstacle j the node's share {fx, fy, fz, in contact} at fk[(j * n_surf + k) * 4].  g (may be null: refresh of
// the buffers only) gains grad Phi.  Pinned nodes (fixed_slot >= 0) take no part.  xp/yp/zp: start-of-step positions.
void launch_obstacle_grad(hipStream_t s, int n_surf, const int* node, const double* w, const ObstacleList& L,
                          const double* x, const double* y, const double* z, const double* xp, const double* yp,
                          const double* zp, double h, const int* fixed_slot, double* g, double* f, double* blk,
                          double* fk);
// H's diagonal block of every surface node += h * block (H = M/h + h K: the same scaling as the element tangent)
void launch_obstacle_hessian(hipStream_t s, int n_surf, const int* node, const int* off, const int* diagpos,
                             const double* blk, double h, double* H);
// out[j][4] = fixed-order sums of fk over the surface nodes, one block per obstacle
void launch_obstacle_resultant(hipStream_t s, int n_surf, int n_obs, const double* fk, double* out);

// The same obstacles on the ANCF kinds (tlfea_ancf_set_obstacles, DESIGN 3e'; ancf_obstacle_kernels.hip): contact at
// kAncfObsPoints sample points per element, spread to the element's coefficients through the shape functions.
constexpr int kAncfObsPoints = 32;
struct AncfObsView {
  int E, S;
  const int* conn;      // [S][E] coefficient ids (ElemView::conn)
  const int* cls;       // [E] the element's (L, W, H) class
  const double* sval;   // [n_class][32][S] shape values S_a(p)
  const double* w;      // [E][32] quadrature weight x reference surface Jacobian
  double* cbuf;         // [E][S][3] contact force rows (the layout of fbuf)
  double* blk;          // [E][32][6] C_p (xx yy zz xy xz yz), written for touched elements only
  double* fk;           // [n_obs][E][4] per obstacle: the element's force share | its points in contact
  int* touched;         // [E] some point has d < 0 or an active friction term
};
// points kernel: fills cbuf, blk, fk and touched from the current (x) and start-of-step (xp) coordinates
void launch_ancf_obstacle_points(hipStream_t s, const AncfObsView& v, const ObstacleList& L, const double* x,
                                 const double* y, const double* z, const double* xp, const double* yp, const double* zp,
                                 double h);
// Kbuf's (i <= j) blocks of every touched element += h sum_p S_i S_j C_p
void launch_ancf_obstacle_tangent(hipStream_t s, const AncfObsView& v, double h, double* Kbuf);
// fc [N][3] = ascending-element sum of the coefficient's cbuf rows; g (may be null) -= fc
void launch_ancf_obstacle_gather(hipStream_t s, int N, const Incidence& inc, const double* cbuf, double* fc, double* g);
// pts [E][32][5] = position | smallest gap | normal pressure sum_j kappa_j <-d_j> of every sample point (a field takes
// part where it covers the point, with kappa <-phi> |G|; a point that nothing covers reports a gap of +inf)
void launch_ancf_obstacle_footprint(hipStream_t s, const AncfObsView& v, const ObstacleList& L, const double* x,
                                    const double* y, const double* z, double* pts);

// Signed distance of a closed triangle surface on a regular grid (tlfea_sdf_from_triangles, DESIGN 3e''; sdf_kernels.hip):
// tri [n_tris][9] vertex coordinates, out the samples first .. first + count - 1 of the nx x ny x nz grid (x fastest).
// One thread per sample, every triangle in ascending order: bitwise reproducible.
constexpr int kSdfTile = 128;  // triangles staged through LDS per tile
void launch_sdf_from_triangles(hipStream_t s, const double* tri, int n_tris, int nx, int ny, const double origin[3],
                               double spacing, long long first, long long count, double* out);

// Distributed loads (tlfea_set_body_acceleration, tlfea_ancf_set_surface_loads; load_kernels.hip).  No atomics.
constexpr int kMaxLoads = 16;
// Faces per element: shell 2, beam 4; pressure points per face P: shell 5 x 5, beam 5 x 2.
struct AncfLoadView {
  int E, S;
  const int* conn;      // [S][E] coefficient ids (ElemView::conn)
  const int* cls;       // [E] the element's (L, W, H) class
  const double* tab;    // [n_class][faces][P][3][S]: S_a(q), dS_a/d(first face direction), dS_a/d(second)
  const double* qw;     // [P] quadrature weight of point q
  const int* mask;      // [E] bit f: some pressure load lists face f of the element
  const double* pe;     // [E][faces] -(sum of scale x pressure over the loads of the face) x the face's orientation sign
  double* lbuf;         // [E][S][3] pressure force rows (the layout of fbuf); written for elements with mask != 0 only
};
// fc [N][3] = sum_j M_ij a_j (+ add, may be null), a_j = a where j % stride == 0 (T10: 1, ANCF: 4); mval null: fc = add
void launch_body_force(hipStream_t s, int N, const Incidence& inc, const double* mval, int stride, const double a[3],
                       const double* add, double* fc);
// lbuf rows of every element with a pressure load, from the current coefficients
void launch_ancf_pressure(hipStream_t s, const AncfLoadView& v, const double* x, const double* y, const double* z);
// Follower pressure on the boundary faces of a T10 mesh (tlfea_t10_set_surface_loads, DESIGN 3h'): the LOADED faces only,
// in ascending face order.  The gather is launch_load_gather with an Incidence whose n2e_off / n2e are the node-to-slot
// CSR of fbuf (slot = loaded face * 6 + local node, ascending per node).
struct T10LoadView {
  int n_faces;          // loaded faces
  const int* nodes;     // [n_faces][6] node ids, ordered outward (corners, then the mid-edge nodes 01 12 02)
  const double* pe;     // [n_faces] -(sum of scale x pressure over the loads of the face)
  double* fbuf;         // [n_faces][6][3] pressure force rows
};
void launch_t10_pressure(hipStream_t s, const T10LoadView& v, const double* x, const double* y, const double* z);
// f [N][3] = fc (may be null) + ascending-element sum of the coefficient's lbuf rows (lbuf may be null); g -= f
void launch_load_gather(hipStream_t s, int N, const Incidence& inc, const double* fc, const double* lbuf, double* f,
                        double* g);

// Stress and energy recovery of T10 objects (tlfea_t10_calc_stress; stress_kernels.hip).  No atomics.
// pts (null: not wanted) [E][5][6] Cauchy stress per Keast point, xx yy zz xy yz zx; erec [E][10] = volume-weighted mean
// stress (6) | its von Mises | mean strain-energy density | mean J | reference volume V_e; contrib [4][Epad] the element's
// integrals of {psi, P_vis:Fdot, 1, J}.  v (3N interleaved, may be null) adds the Kelvin-Voigt stress of a damped material.
void launch_stress_points(hipStream_t s, const ElemView& m, const Material& mat, const double* emat, const double* v,
                          double* pts, double* erec, double* contrib);
// nodal [N][7]: V_e-weighted mean of the incident elements' mean stresses (ascending element order) | its von Mises
void launch_stress_nodal(hipStream_t s, int N, const Incidence& inc, const double* erec, double* nodal);
// The same for the ANCF kinds (tlfea_ancf_calc_stress, DESIGN 3f'): lanes own quadrature points, pts [E][Q][6]; one material
void launch_ancf_stress_points(hipStream_t s, const ElemView& m, const Material& mat, const double* v, double* pts,
                               double* erec, double* contrib);
// nodal [n_nodes][7] over MESH nodes: off [n_nodes + 1] / el = the elements of every node, ascending
void launch_stress_node_gather(hipStream_t s, int n_nodes, const int* off, const int* el, const double* erec,
                               double* nodal);
// out5 = {strain energy, 1/2 v.Mv (0 without v), viscous power, reference volume, current volume}: fixed-order partial
// sums (partial: kStressMaxPart x 5 doubles), then one block with a fixed tree
constexpr int kStressMaxPart = 1024;
void launch_stress_totals(hipStream_t s, int E, int Epad, const double* contrib, int N, const Incidence& inc,
                          const double* mval, const double* v, double* partial, double* out5);

// Recovered nodal stress, principal stresses and the ZZ error indicator of T10 objects (tlfea_t10_recover_stress, DESIGN
// 3f''; stress_recovery_kernels.hip).  No atomics.
struct RecoveryTable {
  double T[kNN][kNQ];   // least-squares linear fit of the rule's point values, evaluated at the element's ten nodes
  double Nq[kNQ][kNN];  // shape functions at the rule's points
  double qw[kNQ];
};
// rec [E][kRecoveryRec] = V_e x the fit at the four vertices (4 x 6) | V_e | 0 | the volume-weighted mean stress (6)
constexpr int kRecoveryRec = 32;
void launch_recovery_elem(hipStream_t s, int E, const double* detJ, const RecoveryTable& tb, const double* pts /*[E][5][6]*/,
                          double* rec);
// nodal [N][7] = sum_e V_e (T[a(e,i)] . sigma_e) / sum_e V_e over the node's elements in ascending order | its von Mises:
// from the element records, or (direct) from the point blocks themselves
void launch_recovery_nodal(hipStream_t s, int N, const Incidence& inc, const double* rec, double* nodal);
void launch_recovery_nodal_direct(hipStream_t s, int N, const Incidence& inc, const RecoveryTable& tb, const double* pts,
                                  const double* rec, double* nodal);
// tensor k = src[k stride + offset ..+6] -> val [n][4] = s1 >= s2 >= s3 | (s1 - s3) / 2, dir (may be null) [n][9] = the unit
// eigenvectors as rows of a right-handed frame; cyclic Jacobi, a fixed number of sweeps
void launch_principal(hipStream_t s, int n, const double* src, int stride, int offset, double* val, double* dir);
// err [3][Epad] = eta_e^2 (clamped at 0) | n_e^2 | 1 where clamped, of the recovered field nodal [N][7] against pts
void launch_zz_error(hipStream_t s, const ElemView& m, const Material& mat, const double* emat, const RecoveryTable& tb,
                     const double* pts, const double* nodal, double* err);

// Adjoint sensitivities of the implicit Newton step of T10 objects (tlfea_newton_adjoint_step, DESIGN 3j;
// adjoint_kernels.hip).  No atomics.
struct SensShape {
  double Nq[kNQ][kNN];  // shape functions at the rule's points (the mass matrix's rule)
};
// sens [P + 1][Epad] per element, P = 2 (SVK: lambda, mu) | 3 (Mooney-Rivlin: mu10, mu01, kappa):
// -sum_q dV (dP/dtheta_p)(F) : grad w, then the density slot -sum_q dV (N w).(N u) (u null: zeros).  w, u [3N] interleaved.
void launch_sens_points(hipStream_t s, const ElemView& m, int model, const SensShape& sh, const double* w, const double* u,
                        double* sens);
// The ANCF kinds (DESIGN 3j'): sens [P][Epad], stiffness slots only; w [3 n_coef] interleaved.  The density slot is
// sum_i out_i of launch_ancf_rho_terms: out [N], out_i = scale (M w)_i . u_i.
void launch_ancf_sens_points(hipStream_t s, const ElemView& m, int model, const double* w, double* sens);
void launch_ancf_rho_terms(hipStream_t s, int N, const double* Mw, const double* u, double scale, double* out);
void launch_sens_transpose(hipStream_t s, int E, int Epad, int slots, const double* sens, double* out /*[E][slots]*/);
// Fixed-order sums of `slots` (1 .. 4) values per item over groups of items: value (c, k) = src[c slot_stride +
// item item_stride], item = idx ? idx[k] : k.  Partial block b adds the items [blk[b].x, blk[b].y) (blk null: chunks of
// kAdjChunk over [0, n)), then block g of the final launch adds the partial rows [boff[g], boff[g + 1]) (boff null: one
// group of all nb rows) into out [groups][slots].  partial: nb x slots doubles.
constexpr int kAdjChunk = 4096;
void launch_adj_sums(hipStream_t s, int slots, int n, int nb, const int2* blk, const int* idx, const double* src,
                     size_t slot_stride, int item_stride, int groups, const int* boff, double* partial, double* out);
// the constraint Jacobian J as the vector kernels see it: mode 0 none, 1 the fixed-node selector (constraint
// 3 slot + c = component c of node fixed[slot]), 2 CSR rows (and J^T in CSR over DOF rows)
struct AdjCons {
  int mode;
  const int *fixed, *fixed_slot;            // mode 1: [n_fixed] nodes, [N] slot of a node or -1
  const int *joff, *jcol, *jtoff, *jtcol;   // mode 2
  const double *jval, *jtval;
};
// x_t = x_bar + rho J^T lam_bar, v_t = v_bar + h x_t, u = (v - v_prev) / h - a over the n = 3N DOFs (null cotangent = 0);
// a acts on every stride-th coefficient vector (T10: 1, every node; ANCF: 4, the position coefficients) and is 0 elsewhere
void launch_adj_rhs(hipStream_t s, int n, const AdjCons& J, const double* xbar, const double* vbar, const double* lambar,
                    const double* v, const double* vprev, const double a[3], int stride, double h, double rho, double* xt,
                    double* vt, double* u);
// f_ext_bar = w, v_prev_bar = M w / h, x_prev_bar = x_t - (v_t - M w / h) / h per DOF; lam_in_bar = lam_bar - h J w,
// t_bar = h rho J w - rho lam_bar per constraint row (null output = not wanted)
void launch_adj_out(hipStream_t s, int n, int nc, const AdjCons& J, const double* w, const double* Mw, const double* xt,
                    const double* vt, const double* lambar, double h, double rho, double* fext_bar, double* vprev_bar,
                    double* xprev_bar, double* lam_in_bar, double* t_bar);

// Shape sensitivities of the implicit Newton step (shape_kernels.hip).  No atomics.
// rows [10][Epad][3] per (local node, element): sum_q dV S_q G_b,q with S = (P : D + rho (N w).(N u)) I - F^T dP[D] - D^T P
// at the current positions; mat.rho0 (emat: slot kEmRhoM of the element's record) is the density of the mass term, u null
// = no mass term; q: the points of the mass matrix's rule (x | y | z).  Then X_bar [N][3] = - the sum of every node's rows in ascending element order.
void launch_shape_points(hipStream_t s, const ElemView& m, const Material& mat, const double* emat, const double q[3][kNQ],
                         const double* w, const double* u, double* rows);
void launch_shape_gather(hipStream_t s, int N, int Epad, const Incidence& inc, const double* rows, double* xbar);

}  // namespace tlfea
