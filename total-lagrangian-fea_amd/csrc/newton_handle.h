// newton_handle.h -- the Newton solver object behind tlfea_newton_t with the level types of its preconditioner, and the
// functions of tlfea_api.hip, partition_api.hip, precond_api.hip, cg_api.hip, adjoint_api.hip, direct_api.hip and
// rccl_api.hip that another unit calls.
// Included by the host units that take a tlfea_newton_t apart; private to csrc/.
#pragma once
#include <map>
#include <tuple>

#include "data_handle.h"

using namespace tlfea;  // as every unit that includes this header says itself: the types below are written in its names

// =================================================================================================
// One single-precision polynomial step (launch_cheb32) takes its operands from three places: the level (C32Level), the
// level's ping-pong vectors (C32Vecs) and the call (rows, coefficient pair, outputs of the last step); c32_step() below.
struct C32Level {
  int nnz;
  Incidence inc;
  const void *B8, *B1;  // the level's low-precision scaled copy, 8 + 1 entries per block
  int bits;
  const double* sc;
  int geo;  // slot of tlfea_newton_s::c32_geo the launch geometry is recorded in; -1: not recorded
};
struct C32Vecs {  // d, z^, res^ and their ping-pong partners (6 x n floats), then (S D S)^-1 (3 n)
  float *d, *d2, *z, *z2, *r, *r2;
  const float* Dinv_f;
  C32Vecs(float* base, size_t n)
      : d(base), d2(base + n), z(base + 2 * n), z2(base + 3 * n), r(base + 4 * n), r2(base + 5 * n), Dinv_f(base + 6 * n) {}
  void swap() { std::swap(d, d2); std::swap(z, z2); std::swap(r, r2); }
};
// partition-boundary nodes of a level (tlfea_newton_set_interface): their rows are summed over ranks
struct LevelIface {
  int n_loc, n_glob;  // boundary nodes on this rank / slots of the exchange buffer
  const int *d_node, *d_slot;
  const int* d_bslot;  // [N] exchange slot of a boundary node, -1 inside
};

// A coarse level of the p-multigrid cycle (vertex level, third level): pattern, operator, block-Jacobi scaling, the
// low-precision copy its polynomial streams, and the work vectors.  The fine level keeps its members in tlfea_newton_s.
struct PolyLevel {
  int N = 0, nnz = 0;  // nodes, 3 x 3 blocks
  int *d_off = nullptr, *d_cols = nullptr, *d_diagpos = nullptr;
  double *d_H = nullptr, *d_D = nullptr, *d_Dinv = nullptr, *d_sc = nullptr, *d_Dinv_s = nullptr;
  double *d_eigv = nullptr, *d_q = nullptr, *d_p = nullptr;  // power iteration: the kept vector and two work vectors
  void *d_B8 = nullptr, *d_B1 = nullptr;
  int bits_alloc = 0;
  float* d_f32 = nullptr;  // C32Vecs(d_f32, 3 N)
  double lam = 0.0;        // lambda_max(D^-1 H) estimate, warm-started across solves
  Incidence inc() const { return Incidence{nullptr, nullptr, nullptr, d_off, d_cols, d_diagpos}; }
  C32Level c32(int bits, int geo) const { return C32Level{nnz, inc(), d_B8, d_B1, bits, d_sc, geo}; }
  int alloc_work() {  // once N and nnz are known
    const size_t n = 3 * (size_t)N;
    TRY(dmalloc(&d_H, (size_t)9 * nnz));
    TRY(dmalloc(&d_D, (size_t)9 * N)); TRY(dmalloc(&d_Dinv, (size_t)9 * N));
    TRY(dmalloc(&d_sc, n)); TRY(dmalloc(&d_Dinv_s, (size_t)9 * N));
    TRY(dmalloc(&d_eigv, n)); TRY(dmalloc(&d_q, n)); TRY(dmalloc(&d_p, n));
    TRY(dmalloc(&d_f32, 6 * n + (size_t)9 * N));
    return 0;
  }
  int ensure_copy(int bits) {  // storage of the low-precision copy at `bits` per entry
    if (bits_alloc == bits) return 0;
    if (d_B8) (void)hipFree(d_B8);
    if (d_B1) (void)hipFree(d_B1);
    d_B8 = d_B1 = nullptr;
    HIP_TRY(hipMalloc(&d_B8, (size_t)nnz * 8 * (bits / 8)));
    HIP_TRY(hipMalloc(&d_B1, (size_t)nnz * (bits / 8)));
    bits_alloc = bits;
    return 0;
  }
  void release() {
    void* p[] = {d_off, d_cols, d_diagpos, d_H, d_D, d_Dinv, d_sc, d_Dinv_s, d_eigv, d_q, d_p, d_B8, d_B1, d_f32};
    for (void* q : p)
      if (q) (void)hipFree(q);
    *this = PolyLevel();
  }
};

struct tlfea_newton_s {
  tlfea_t10_t d = nullptr;
  int N = 0, n_constraints = 0;
  bool cons_enabled = false;     // constructed with n_constraints > 0: the reference gates every constraint term on it
  int n_constraints_global = 0;  // over all ranks (control flow must be identical on every rank)
  tlfea_newton_params prm{1e-4, 1e-4, 1e-4, 1e14, 5, 10, 1e-3};
  tlfea_linsolve_opts lin{1e-12, 20000, 25, 0, 0.0, 0, 0, 0, 0};
  double lin_last_rel = 0.0, lin_worst_rel = 0.0;  // ||r||/||b|| of the last linear solve / the worst since the step began
  bool lin_last_ok = true, lin_all_ok = true;
  double lam_max = 0.0;       // estimate of lambda_max(D^-1 H) (power iteration, warm-started across solves)
  double lam_safety = 1.15;   // the polynomial's interval ends at lam_safety * lam_max (power iteration converges from below)
  double* d_eigv = nullptr;   // its vector
  double *d_cd = nullptr, *d_cd2 = nullptr, *d_cres = nullptr;  // Chebyshev work vectors
  // low-precision scaled copy of H streamed by the Chebyshev steps (lin.cheb_bits 16/32): 8+1 entries per block
  void *d_B8 = nullptr, *d_B1 = nullptr;
  int lp_bits_alloc = 0;
  // The copy belongs to the H, d_sc and d_D of ONE stage-0 set-up (precond_setup): lp_scaled = that stage ran the scaling,
  // lp_current = the copy was converted from them since, lp_converts = fine-level conversions since creation.  A set-up
  // that can still choose the matrix-free fine smoother defers the conversion (ensure_fine_copy, DESIGN 3g').
  bool lp_scaled = false, lp_current = false;
  int lp_converts = 0;
  double *d_sc = nullptr, *d_Dinv_s = nullptr;
  double *d_cz = nullptr, *d_cz2 = nullptr, *d_cres2 = nullptr;  // ping-pong partners of z / res in the LP steps
  // two-level p-multigrid preconditioner (T10, single GPU): see pmg_host.h / pmg_apply()
  struct Pmg {
    bool tried = false, ok = false;
    PolyLevel vertex;  // the vertex level: Hc = P^T H P
    int *d_par0 = nullptr, *d_par1 = nullptr, *d_cblk_row = nullptr, *d_child_off = nullptr, *d_child = nullptr,
        *d_con_off = nullptr, *d_con_base = nullptr, *d_con_deg = nullptr;
    int n_upper = 0;  // Galerkin gather: blocks with column >= row (d_c_upper), the rest mirrored through d_c_mirror
    int *d_c_upper = nullptr, *d_c_mirror = nullptr;
    float *d_child_w = nullptr, *d_con_w = nullptr;
    // T10: Hc from an image of the R row (pmg_host.h GalRowsHost, pmg_galerkin_rows_kernel) -- the ONE arithmetic of every
    // conforming T10 set-up whose lists fit; the gather lists above are then not on the device.  The row structure it walks
    // is rop's (d_off .. d_ch_w, d_pos_off, d_con_pos), up whether or not R itself is built.
    struct Rows {
      bool ok = false;
      int *d_row = nullptr, *d_off = nullptr, *d_long_rows = nullptr;
      unsigned short* d_pos = nullptr;
      unsigned char* d_w = nullptr;
      int cap = 0, n_long = 0, ws_rows = 0;  // image capacity in blocks; the rows beyond it, and how many a launch takes
      size_t ws_stride = 0;                  // doubles per slice of d_ws: nine times the longest of them
      double* d_ws = nullptr;
    } rows;
    // which kernel of the last set-up left vertex.d_H: 1 the gather, 2 the row kernel alone, 3 fused with the build of R;
    // 0: no set-up yet, or a read-back has summed Hc again since
    int hc_form = 0;
    double* d_coef = nullptr;  // the cycle's coefficient table (pmg_coef.h, PmgTable), kPmgTableCap doubles
    // multi-GPU: the coarse level is partitioned like the fine one (vertex nodes of the partition boundary are
    // replicated); slots of the coarse exchange buffer are agreed once (pmg_prepare), child weights carry 1/multiplicity
    int n_ifc_loc = 0, n_ifc_glob = 0;
    int Nc_glob = 0;                  // coarse nodes over all ranks: what the coarse polynomial's degree goes by (every
                                      // rank must run the same number of steps -- each is a collective)
    int *d_ifc_node = nullptr, *d_ifc_slot = nullptr, *d_bslot_c = nullptr;
    double* d_wc3 = nullptr;          // [3 Nc] 1/multiplicity of the coarse DOFs
    float* d_child_w_dist = nullptr;  // child weights x 1/multiplicity of the child
    // the coarse polynomial's degree is a size-based guess (fitted on configs B, C); when a solve stalls because the
    // vertex-level operator is worse conditioned than the guess covers (a 5 x 3.3 x 1.7 bar of 4.5 M elements needs
    // degree ~50 where the guess says 39), the solver raises it for this and all later solves
    double kc_boost = 1.0;
    // restricted fine operator R = S_c P^T S_f^-1 Hs (pmg_host.h pmg_restrict_op_build; one GPU, first-kind smoother):
    // pattern and contribution lists with the hierarchy, values (fp32, 8 + 1 per block) rebuilt by pmg_build_level
    struct Rop {
      bool ok = false, built = false;
      int nnz = 0, n_con = 0;
      int *d_off = nullptr, *d_cols = nullptr, *d_ch_off = nullptr, *d_ch = nullptr, *d_con_off = nullptr,
          *d_con_blk = nullptr;
      unsigned char* d_con_ord = nullptr;
      float *d_ch_w = nullptr, *d_R1 = nullptr;
      void* d_R8 = nullptr;
      // positions by source, for the kernels that stream each child's row of H (Rows); stream_cap > 0: a matrix-free
      // set-up builds R in that pass too
      int* d_pos_off = nullptr;
      unsigned short* d_con_pos = nullptr;
      int stream_cap = 0;
    } rop;
    LevelIface iface() const { return LevelIface{n_ifc_loc, n_ifc_glob, d_ifc_node, d_ifc_slot, d_bslot_c}; }
    // third level: rigid-body-mode aggregates of the vertex level (pmg_host.h agg_build); lvl.N = 2 Na nodes
    struct Agg {
      bool ok = false, bins = false;
      double size_ratio = 0.0;  // bins: cell size in mean vertex edges (0: greedy aggregates, ~2.2)
      double* d_r3 = nullptr;  // overlapping partition: this rank's share of the level-3 residual (summed over ranks)
      int Na = 0, n_pairs = 0;
      PolyLevel lvl;           // H3 = P2^T Hc P2
      int *d_agg = nullptr, *d_active = nullptr, *d_mem_off = nullptr, *d_mem = nullptr, *d_pair_A = nullptr,
          *d_pair_pos = nullptr, *d_pair_B = nullptr, *d_pcon_off = nullptr, *d_pcon_base = nullptr, *d_pcon_deg = nullptr,
          *d_pcon_i = nullptr, *d_pcon_j = nullptr;
      double* d_rvec = nullptr;
    } agg;
  } pmg;
  LevelIface iface() const { return LevelIface{n_if_loc, n_if_glob, d_if_node, d_if_slot, d_bslot_f}; }
  float* d_f32 = nullptr;  // single-precision polynomial (single GPU): d, z, res ping-pong pairs (6 x 3N) + (SDS)^-1 (9N)
  bool fixed_pattern = false, sparsity_done = false;
  int verbose = 0;
  // Launch stream.  Single GPU: an own (blocking) stream, so that the CG iteration can be captured as a hipGraph
  // (the legacy default stream cannot be captured; a blocking stream still orders against the data object's
  // default-stream copies and kernels).  With a multi-GPU interface set: the default stream, the one the host's
  // collective (torch.distributed) orders against.
  hipStream_t stream = nullptr, stream_own = nullptr;
  double *d_v = nullptr, *d_vprev = nullptr, *d_lam = nullptr, *d_g = nullptr, *d_dv = nullptr, *d_r = nullptr,
         *d_b = nullptr;
  double *d_step0 = nullptr, *d_lam0 = nullptr;  // v | v_prev and lambda at the start of the running step (roll-back)
  int lam0_cap = 0;
  // what the last Solve() left for tlfea_newton_adjoint_step: 0 no Solve yet, 1 one outer iteration whose Newton loop met
  // its tolerance, 2 more than one outer iteration, 3 the step failed, 4 the Newton loop ran out of iterations
  int adj_state = 0;
  bool profiling = false;  // per-stage hipEvent timing (adds a host sync per stage)
  int pcg_fused = -1;  // -1 auto (fused direction update below 200k nodes), 0/1 forced (TLFEA_PCG_FUSED)
  bool spmv_nt = false; // non-temporal loads of H in the SpMV (TLFEA_SPMV_NT): measured slower at config C
  double *d_xp = nullptr, *d_yp = nullptr, *d_zp = nullptr;
  double *d_H = nullptr, *d_Kbuf = nullptr, *d_Dinv = nullptr;
  // fused tangent + assembly (T10, SVK): row groups (rowgroup_host.h) and the per-point F of the last residual launch.
  // asm_mode (TLFEA_ASSEMBLE=kbuf|direct): 0 auto = fused where it applies, 1 always the two-kernel path via Kbuf
  RowGroups rg{0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int* d_rg[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool rg_ok = false;
  bool fq_in_residual = true;  // first-order solvers (AdamW, Nesterov, VBD) never assemble: their residual skips Fq
  int asm_mode = 0;
  int rg_passes = 0, rg4_passes = 0;  // entries of the pass tables of rg / rg4
  // nodes whose row of H is empty (no element, no general linear constraint row): the first and how many (analyze_hessian_sparsity)
  int iso_first = -1, iso_count = 0;
  double* d_Fq = nullptr;
  // affine-element form of the fused kernel (straight-sided elements + the 5-point Keast rule): its work lists, the
  // per-element vertex gradients; d_Fq then holds F per point, [E][5][10].  TLFEA_ASSEMBLE=general keeps the general form.
  RowGroups4 rg4{0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
  int* d_rg4[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  AffineView av{nullptr, 0, {0, 0, 0, 0}};
  double* d_gvec = nullptr;
  double* d_cmass = nullptr;  // [10][16] element mass coefficients in the kernel's (row node, vertex n, p) order
  bool affine_ok = false;
  long geom_gen_seen = -1;   // data->geom_gen the affine cache (gvec, affine_ok) was built from
  double affine_dev = -1.0;  // largest relative deviation from the affine form found at set-up (-1: not checked)
  // Matrix-free product of the CG iteration: q = H p from gvec and the F records in d_Fq instead of the CSR
  // stream.  `valid`: d_Fq, gvec and the scalars below are those H was assembled from -- set by the affine assembly,
  // cleared by every residual launch that rewrites d_Fq (the next assembly sets it again) and by a new affine set-up.
  struct Matfree {
    bool valid = false;
    MatfreeCoef mc{};
    const int* fixed = nullptr;  // pinned rows of the assembled H (null: none)
    double penalty = 0.0;
    double* d_ybuf = nullptr;    // [10][Epad][3] element rows, allocated on first use; compact form: [rows][3]
    // compact form (matfree_compact.h, TLFEA_MATFREE_COMPACT): the lists, built and uploaded with d_ybuf
    bool compact = false;
    MatfreeCompact cp{nullptr, nullptr, nullptr, nullptr, nullptr};
    void* d_cp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    long cp_rows = 0;
    double cp_ratio = 0.0;       // 10 E / rows
    bool now = false;           // the running / last solve takes the matrix-free product
    int last_mode = 0;           // tlfea_newton_get_spmv_mode
    long gen = 0;                // counts the assemblies that claimed the records (fine smoother: whose records its copies are)
    // packed lane-major fp64 copies the product reads (matfree_records.h): g of the current affine set-up (gp_ok), F of
    // assembly rec_gen; a product that finds another assembly fails
    double *d_gp = nullptr, *d_Fp = nullptr;
    bool gp_ok = false;
    long rec_gen = -1;
  } mf;
  // Fine smoother of the p-multigrid cycle from the element records (DESIGN 3g'): float copies of gvec and d_Fq, the
  // normalised scaling, and the choice the last preconditioner set-up took.  The copies belong to assembly `gen`; an
  // application that finds mf.valid cleared or another assembly fails (pmg_apply).
  struct FineMf {
    bool now = false;            // the last preconditioner set-up chose it (taken once, before R is built)
    int last = 0;                // tlfea_newton_get_fine_smoother
    long gen = -1;               // mf.gen the float F records were converted at
    bool g_ok = false;           // the float g records are those of the current affine set-up
    float *d_g32 = nullptr, *d_F32 = nullptr, *d_scn = nullptr;  // g and F packed (matfree_records.h)
    double* d_ss = nullptr;      // sum(sc^2)
    FineMatfree v{};
  } fmf;
  // Solve set-up from the element records (DESIGN 3g', TLFEA_SETUP_RECORDS): where nothing of a solve reads the CSR H, the
  // Newton loop's assemble() leaves H unassembled and writes instead the image rows of R (d_img, 9 rop.nnz doubles, H's row
  // layout at 9 rop.d_off[I]) and the fine block diagonal (d_D); pmg_build_level sums Hc, D_c, sc_c and R from the image.
  // h_current: d_H holds the H of the last assembly.  Whoever reads d_H calls hessian_current() first, which assembles it
  // from the point records while they are still that assembly's (gen == mf.gen, mf.valid) and fails otherwise.
  struct SetupRec {
    bool tried = false, ok = false;  // the coarse work lists: built once per mesh, and they fit
    RowGroups4 rg{0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
    int* d_rg[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int passes = 0, n_ch = 0;
    double* d_cmass4 = nullptr;      // [4][16] (pmg_host.h image_mass_table)
    int *d_ch_row = nullptr, *d_ch_pos = nullptr, *d_id_off = nullptr, *d_id_ch = nullptr;
    float* d_id_w = nullptr;
    unsigned short* d_id_pos = nullptr;
    double *d_img = nullptr, *d_dbuf = nullptr;  // the image rows; the elements' diagonal blocks [10][Epad][6]
    bool h_current = true;           // (true before any assembly: the readers keep their own "no H yet" checks)
    long gen = -1;                   // mf.gen of the assembly that wrote d_img and d_D from the records
    long n_asm = 0;                  // assemblies of H since the solver was created
    int last_form = 0;               // the last set-up summed Hc and R from: 0 the CSR H, 1 the image
  } sr;
  // sparse direct solve (lin.method == 1): rocSOLVER re-factorisation on a host-computed ordering + factor pattern
  struct Direct {
    bool tried = false, ok = false;
    int backend = 0;  // 0: the engine's multifrontal Cholesky (direct_kernels.hip), 1: rocSOLVER (TLFEA_DIRECT_BACKEND=rocsolver)
    int n = 0, nnzT = 0;
    void *blas = nullptr, *rfinfo = nullptr;
    int *d_ptrA = nullptr, *d_indA = nullptr, *d_ptrT = nullptr, *d_indT = nullptr, *d_pivQ = nullptr;
    double* d_valT = nullptr;
    MfPlan plan;      // host plan (levels, panel steps); the device copies below
    MfDev dev{};
    MfTally tally;    // launches of the last native factorisation + solve (tlfea_newton_get_direct_info)
    std::vector<void*> owned;  // device allocations of the native backend
    double factor_ms = 0.0, solve_ms = 0.0;
  } direct;
  double* d_mbuf = nullptr;   // T10: per (element, node) force row | inertia row M_e (v - v_prev) / h of the residual launch
  int mass_mode = 0;          // TLFEA_MASS=csr: always the mass CSR product in grad_kernel
  double *d_p = nullptr, *d_p2 = nullptr, *d_q = nullptr, *d_zv = nullptr;
  double* d_parts = nullptr;  // 6 x kNPart: rz[2], pq, rr, bb, norm
  // read-back hook (tlfea_newton_get_c32_geometry): the last NON-FINAL polynomial step launched on the fine level [0],
  // the vertex level [1] and the third level [2]; regime -1 = none yet
  C32Geometry c32_geo[3] = {{-1}, {-1}, {-1}};
  C32Geometry* geo_out(int level, bool last) { return last ? nullptr : &c32_geo[level]; }
  double* d_scal = nullptr;   // 4 scalars
  double* h_pin = nullptr;    // pinned host words: [0..7] scalars read back, [8..] Chebyshev coefficients to upload
  double* d_coef = nullptr;   // Chebyshev coefficients on the device (2 per step)
  hipGraphExec_t cg_graph[3] = {nullptr, nullptr, nullptr};  // CG iteration of even / odd parity / odd + residual replacement
  // Mixed-precision outer iteration (single GPU, fp32 polynomial path): the CG's SpMV streams a single-precision copy of
  // H (half the bytes of the iteration's largest launch); every `spmv32_every` iterations -- and before convergence is
  // declared -- the residual is replaced by b - H x in fp64 on H itself (reliable updates), so the attained residual
  // and the stopping test are those of the fp64 system.  OPT-IN (TLFEA_SPMV32 = replacement period, even; 0 = off = the
  // default): measured at config C it saves 2.6 % of a Newton iteration with period 8, stagnates at 5e-11 with period
  // 16, and on ill-conditioned systems (welded ANCF net, penalty 1e14: cond(H) eps_fp32 > 1) it stagnates at 7e-9 --
  // each replacement restarts from the error of the fp32 copy.  Kept as an experiment switch, not a default.
  float* d_H32 = nullptr;
  int spmv32_every = 0;
  bool spmv32_now = false;       // this solve runs the mixed-precision iteration
  const double* cur_b = nullptr; // right-hand side of the running solve (residual replacement)
  long n_replacements = 0;
  long cg_graph_key[6] = {0, 0, 0, 0, 0, 0};
  // test hook tlfea_newton_cg_trace: while set, pcg() runs exactly `k` iterations without convergence tests and copies the
  // iterates to the host after its start and after every iteration (cg_trace_record)
  struct CgTrace {
    int k = 0;
    double *vecs = nullptr, *sums = nullptr, *slots = nullptr;  // host: [(k+1)][5][3N], [(k+1)][4], [(k+1)][5][kNPart]
    int* form = nullptr;                                        // host: kCgTraceForm ints
  };
  CgTrace* trace = nullptr;
  bool use_graphs = true;     // TLFEA_GRAPH=0 launches every kernel eagerly
  int last_outer_iters = 0;   // CG iterations of the previous solve: where the next one starts testing convergence
  // ANCF: 12 x 12 node-block scaling of the polynomial's operator (solver_kernels.hip, blk12_*): -1 not decided yet
  int blk12 = -1;
  double* d_L12inv = nullptr;
  float* d_L12inv_f = nullptr;
  int* d_blk12_err = nullptr;
  int last_deg = 0, last_bits = 0;
  int h_nnz = 0;
  std::vector<int> h_row_offsets, h_col_indices;  // reference DOF-level CSR index arrays (host)
  double stats[6] = {0, 0, 0, 0, 0, 0};
  double stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double stage_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t ev[8] = {nullptr};
  // multi-GPU interface
  int n_if_loc = 0, n_if_glob = 0;  // local interface nodes / slots of the global exchange buffer
  int *d_if_node = nullptr, *d_if_slot = nullptr;
  int* d_bslot_f = nullptr;         // [N] exchange slot of a partition-boundary node, -1 inside
  std::vector<int> h_if_node, h_if_slot;
  std::vector<double> h_nw;
  long n_collectives = 0;           // all-reduce calls since the solver was built (tests: collectives per CG iteration)
  double *d_ibuf = nullptr, *d_w = nullptr, *d_nw = nullptr, *d_wc = nullptr, *d_D = nullptr;
  // rank-local polynomial preconditioner (multi-GPU): 1 for the nodes this rank owns (every replicated node has
  // exactly one owner), and the scaling vector masked by it
  int* d_own = nullptr;
  double* d_sc_mask = nullptr;
  double lam_max_loc = 0.0;
  bool lmax_mf_ok = false;    // set by pcg() around its own set-up call: the fine lambda_max product may be matrix-free
  bool lmax_used_mf = false;  // the last fine estimate used the matrix-free product (tlfea_newton_get_lambda_max)
  double hook_lam[3] = {0.0, 0.0, 0.0};  // lambda_max estimates of the last tlfea_newton_apply_preconditioner set-up
  bool sync_before_cb = true;
  tlfea_allreduce_fn ar = nullptr;
  void* ar_user = nullptr;
  // Overlapping partition (tlfea_newton_set_halo): owner-computes with ghost layers.  `ar` stays null -- no boundary
  // sums exist -- so every launch sequence is the single-GPU one; the hooks are ghost refreshes, owner-weighted dot
  // products summed with halo.arfn, and row counts that stop at the layers a launch can still compute correctly.
  struct HaloPlan {   // "refresh ghost layers <= D" of one level: concatenated per-peer prefixes of the send / recv lists
    int n_send = 0, n_recv = 0;
    int *d_sidx = nullptr, *d_ridx = nullptr;
    std::vector<long long> soff, roff;   // [n_peers + 1], in nodes
  };
  struct HaloLevel {  // per-peer segments, each ordered by (layer on the receiving side, global id)
    std::vector<int> send_off, send_nodes, send_layer, recv_off, recv_nodes, recv_layer;
    std::map<int, HaloPlan> plans;
  };
  struct Halo {
    bool on = false, native = false;
    int depth = 0, rank = 0, world = 0;
    std::vector<int> peers, layer, n_upto;   // n_upto[k] = local nodes of layers <= k (k = 0 .. depth)
    std::vector<int> n_upto_c;               // the same for the coarse (vertex) level
    HaloLevel lv[2];                         // 0 fine, 1 coarse
    void *d_sbuf = nullptr, *d_rbuf = nullptr;
    size_t cap_s = 0, cap_r = 0;
    double* d_red = nullptr;                 // staging of the reduction slots
    tlfea_halo_exchange_fn xfn = nullptr;
    tlfea_allreduce_fn arfn = nullptr;
    void* user = nullptr;
    bool sync_cb = true;
    long n_exch = 0, n_allred = 0, n_cg_iters = 0, n_exch_cg = 0, n_allred_cg = 0;
    double bytes_exch = 0.0, bytes_allred = 0.0, comm_ms = 0.0;
    bool in_cg = false;                       // inside enqueue_cg_iteration: what the per-iteration budget counts
    double graph_cost[3][5] = {{0}};          // per captured graph: exchanges, all-reduces, bytes, bytes, iterations (added per replay)
    std::vector<long long> so_b, ro_b;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int rows(int k) const { return n_upto[std::max(0, std::min(k, depth))]; }
    int rows_c(int k) const { return n_upto_c[std::max(0, std::min(k, depth))]; }
  } halo;
};

struct StageTimer {  // hipEvent pair on the launch stream around one stage (profiling mode only)
  tlfea_newton_t s;
  int stage;
  StageTimer(tlfea_newton_t s_, int st) : s(s_), stage(st) {
    if (s->profiling) (void)hipEventRecord(s->ev[0], s->stream);
  }
  void stop() {
    if (!s->profiling) return;
    (void)hipEventRecord(s->ev[1], s->stream);
    (void)hipEventSynchronize(s->ev[1]);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, s->ev[0], s->ev[1]);
    s->stage_ms[stage] += ms;
    s->stage_n[stage] += 1;
  }
};

namespace tlfea {

inline bool dist_on(tlfea_newton_t s) { return s->ar != nullptr || s->halo.on; }
inline double* part(tlfea_newton_t s, int k) { return s->d_parts + (size_t)k * kNPart; }

// device scratch of one call, released when the call returns
struct ModalWork {
  std::vector<void*> owned;
  ~ModalWork() {
    for (void* p : owned)
      if (p) (void)hipFree(p);
  }
  int alloc(double** p, size_t n) {
    TRY(dmalloc(p, n));
    owned.push_back(*p);
    return 0;
  }
};
// Warm-start state of the lambda_max estimates (fine level and the coarse levels that exist): save() keeps it and sets the
// estimates cold, so that what follows depends on no earlier solve; restore() puts it back.  A level built in between did
// not exist at the save: its vector stays, its estimate goes back to 0.  solve_state: a call that runs solves of its own
// (modal solve, adjoint step) also keeps the scalars a linear solve leaves for the next one and for the status read-backs.
struct LamKeep {
  std::vector<std::pair<double*, size_t>> vecs;  // the kept vectors that exist at the save
  std::vector<std::pair<double*, double>> lams;  // the estimates
  double* d_save = nullptr;
  tlfea_newton_t kept_of = nullptr;              // solve_state: the solver whose scalars `kept` holds
  std::tuple<double, double, int, int, int, int, double, double, bool, bool> kept;
  static auto solve_scalars(tlfea_newton_t s) {
    return std::tie(s->lam_safety, s->pmg.kc_boost, s->last_outer_iters, s->last_deg, s->last_bits, s->mf.last_mode,
                    s->lin_last_rel, s->lin_worst_rel, s->lin_last_ok, s->lin_all_ok);
  }
  int save(tlfea_newton_t s, ModalWork& wk, bool solve_state = false) {
    size_t total = 0;
    for (PolyLevel* L : {&s->pmg.vertex, &s->pmg.agg.lvl})
      if (L->d_eigv) vecs.push_back({L->d_eigv, 3 * (size_t)L->N});
    vecs.push_back({s->d_eigv, 3 * (size_t)s->N});
    for (auto& v : vecs) total += v.second;
    TRY(wk.alloc(&d_save, total));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(copy(true));
    for (double* p : {&s->lam_max, &s->lam_max_loc, &s->pmg.vertex.lam, &s->pmg.agg.lvl.lam}) {
      lams.push_back({p, *p});
      *p = 0.0;
    }
    if (solve_state) {
      kept_of = s;
      kept = solve_scalars(s);
    }
    return 0;
  }
  void restore() {
    for (auto& l : lams) *l.first = l.second;
    if (kept_of) solve_scalars(kept_of) = kept;
    (void)copy(false);
  }
  hipError_t copy(bool out) {
    hipError_t e = hipSuccess;
    double* at = d_save;
    for (auto& v : vecs) {
      const hipError_t e1 = hipMemcpy(out ? at : v.first, out ? v.first : at, v.second * sizeof(double), hipMemcpyDeviceToDevice);
      if (e == hipSuccess) e = e1;
      at += v.second;
    }
    return e;
  }
};

// partition_api.hip: the partition plumbing
bool halo_graph_wanted();
void halo_graph_give_up();  // RCCL cannot be captured / replayed here: eager launches for the rest of the process
int halo_dr(tlfea_newton_t s);
void halo_free_plans(tlfea_newton_s::HaloLevel& L);
int halo_refresh_f64(tlfea_newton_t s, int level, int D, int dim, double* a, double* b = nullptr, double* c = nullptr);
int halo_refresh_f32(tlfea_newton_t s, int level, int D, int dim, float* a, float* b = nullptr, float* c = nullptr);
int call_allreduce(tlfea_newton_t s, double* d_buf, int n);
int allreduce_host(tlfea_newton_t s, double* d_buf, double* h, size_t n);
int iface_sum_lvl(tlfea_newton_t s, const LevelIface& I, double* d_vec, int dim, double* d_extra = nullptr,
                  int n_extra = 0, double* d_extra2 = nullptr);
int iface_sum(tlfea_newton_t s, double* d_vec, int dim, double* d_extra = nullptr, int n_extra = 0,
              double* d_extra2 = nullptr);
int parts_sum(tlfea_newton_t s, double* d_a, double* d_b = nullptr);
int device_sumsq_async(tlfea_newton_t s, const double* d_vec, const double* w, int n);
int fetch_scalar(tlfea_newton_t s, const double* d_src, double* out);
int fetch_scalar2(tlfea_newton_t s, const double* d_src, double* out0, double* out1);
int device_norm(tlfea_newton_t s, const double* d_vec, const double* w, int n, double* out);
// tlfea_api.hip: the Newton solver's element stage and the fp64 matrix-free product
int refuse_empty_rows(tlfea_newton_t s, const char* who);
int sync_constraints(tlfea_newton_t s);
bool pinned_on(tlfea_newton_t s);
bool lincons_on(tlfea_newton_t s);
void shape_at_rule_points(tlfea_t10_t d, double Nq[kNQ][kNN]);
bool matfree_eligible(tlfea_newton_t s);
bool matfree_chosen(tlfea_newton_t s);
bool matfree_compact_env();
int matfree_points(bool single);
int matfree_ensure_buffer(tlfea_newton_t s);
int matfree_ensure_records(tlfea_newton_t s);
int launch_matfree_product(tlfea_newton_t s, const double* p, double* q, double* pq_part);
// lazy: the Newton loop's call -- where the solve's set-up can run from the element records (setup_records_decide) H is
// left unassembled and the image rows of R and the fine block diagonal are written instead
int assemble(tlfea_newton_t s, bool fq_fresh = true, bool lazy = false);
// Every reader of s->d_H calls this first: no-op while d_H holds the H of the last assembly, else H is assembled now from
// the point records if they are still that assembly's; fails otherwise, and inside a stream capture.
int hessian_current(tlfea_newton_t s);
// precond_api.hip: the solve set-up from the element records (DESIGN 3g')
int setup_records_decide(tlfea_newton_t s, bool* on);  // after the records are claimed (mf.valid): may this assembly skip H?
int setup_records_assemble(tlfea_newton_t s);          // the image rows of R and d_D from the records
bool setup_records_live(tlfea_newton_t s);             // H is not assembled and d_img / d_D are those of the current records
// precond_api.hip: the preconditioners
struct PmgTable;  // pmg_coef.h
int cheb_degree_eff(tlfea_newton_t s);
int cheb_bits_eff(tlfea_newton_t s);
int precond_eff(tlfea_newton_t s);
bool blk12_now(tlfea_newton_t s);
int cheb_upload_coefficients(tlfea_newton_t s);
int pmg_coarse_degree_eff(tlfea_newton_t s);
int pmg_ks(tlfea_newton_t s);
PmgTable pmg_table(tlfea_newton_t s);
C32Level fine_c32(tlfea_newton_t s);
void c32_step(tlfea_newton_t s, const C32Level& L, C32Vecs& v, int rows, const double* coef, const double* d_r, double* d_z,
              double* rz_part, bool last, C32Bnd bnd = C32Bnd());
int ensure_fine_copy(tlfea_newton_t s);
bool pmg_rop_now(tlfea_newton_t s);
long fine_matfree_key(tlfea_newton_t s);
bool fine_matfree_live(tlfea_newton_t s);
int pmg_coefficients(tlfea_newton_t s);
int precond_apply(tlfea_newton_t s, const double* d_r, double* d_z, double* rz_part, bool init_done);
int precond_setup(tlfea_newton_t s, const double* d_b, int stage);
// stages 0 and 1 back to back from the start vector d_b, then the check of the 12 x 12 node blocks; `who` leads the message
int precond_setup_whole(tlfea_newton_t s, const double* d_b, const char* who);
// cg_api.hip
void cg_graphs_destroy(tlfea_newton_t s);
int pcg(tlfea_newton_t s, const double* d_b, double* d_x, int* iters_out, double* rel_out);
// The adjoint step of the implicit Newton step (DESIGN 3j, 3j') is one function for every element kind; the kind supplies
// what differs.  adjoint_api.hip holds the step and the T10 kind, ancf_adjoint_api.hip the ANCF kind.
struct AdjointKind {
  const char* what;                        // the entry point's name in messages
  int stride;                              // the position coefficients are every stride-th coefficient vector (T10: 1, ANCF: 4)
  int (*refusal)(tlfea_newton_t s);        // why the step cannot run on the solver's state now (0: it can)
  int (*prepare)(tlfea_t10_t d);           // the buffers `materials` writes to
  // enqueues the material slots from the device vectors w, u = (v - v_prev)/h - a and M w: per_material (device, null: not
  // wanted) and per_element (the same)
  void (*materials)(tlfea_t10_t d, hipStream_t st, const double* w, const double* u, const double* Mw, double* per_material,
                    double* per_element);
  size_t (*pm_doubles)(tlfea_t10_t d);     // doubles of per_material and per_element
  size_t (*pe_doubles)(tlfea_t10_t d);
};
int adjoint_step_device(tlfea_newton_t s, const AdjointKind& K, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out,
                        double* X_bar, int* info, double* rel_res);
int adjoint_step_host(tlfea_newton_t s, const AdjointKind& K, const tlfea_adjoint_in* in, const tlfea_adjoint_out* out,
                      double* X_bar, int* info, double* rel_res);
int adjoint_refusal_terms(tlfea_newton_t s, const std::string& w);  // damping, friction, follower pressure, a partitioned mesh
int adjoint_refusal_state(tlfea_newton_t s, const std::string& w);  // what the last Solve() left
int sens_buffers(tlfea_t10_t h);  // d_sn_sens, d_sn_out, d_sn_part and the per-material element lists
// direct_api.hip
void direct_destroy(tlfea_newton_t s);
int direct_solve(tlfea_newton_t s, const double* d_b, double* d_x, int* iters_out, double* rel_out);
// rccl_api.hip: the stream the built-in callbacks enqueue on (the engine sets it around every call of a callback)
extern thread_local hipStream_t g_rccl_stream;

}  // namespace tlfea
