"""SyncedNewtonSolver -- host mirror of lib_src/solvers/SyncedNewton.cuh:35-405 on the C-ABI."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from .binding import (ALLREDUCE_FN, AdamWParamsC, AdjointInC, AdjointOutC, LinSolveOptsC, ModalOptsC, NesterovParamsC, NewtonParams, TlfeaError,
                      VbdParamsC, check, dp, ip, load_library)


@dataclass
class SyncedNewtonParams:  # SyncedNewton.cuh:29-33 (same field order)
    inner_atol: float = 1e-4
    inner_rtol: float = 1e-4
    outer_tol: float = 1e-4
    rho: float = 1e14
    max_outer: int = 5
    max_inner: int = 10
    time_step: float = 1e-3


@dataclass
class LinSolveOpts:
    rel_tol: float = 1e-12
    max_iter: int = 20000
    check_every: int = 25
    cheb_degree: int = 0      # Chebyshev polynomial preconditioner degree (1 = block-Jacobi, 0 = auto = 24)
    cheb_kappa: float = 0.0   # polynomial interval [lmax/kappa, lmax] of D^-1 H (0 = auto, by degree)
    cheb_bits: int = 0        # matrix precision of the polynomial's steps: 64 | 32 | 16 (0 = auto = 16)
    precond: int = 0          # 0 auto | 1 Chebyshev polynomial | 2 two-level p-multigrid (T10, one GPU)
    method: int = 0           # 0 preconditioned CG | 1 sparse direct (where built)
    on_unconverged: int = 0   # 0: a solve that misses rel_tol fails the call (nothing applied) | 1: accept the iterate


@dataclass
class ModalResult:
    """What ModalAnalysis returns: omega2 [n_modes] (rad^2/s^2, ascending), freq_hz = sqrt(max(omega2, 0)) / 2 pi,
    modes [n_modes, N, 3] M-normalised, residuals [n_modes] = ||K phi - omega2 M phi|| / ((omega2 + shift) ||M phi||),
    iterations, converged (modes that met tol), block (columns iterated), precond (0 block-Jacobi, 1 polynomial,
    2 p-multigrid)."""
    omega2: np.ndarray
    freq_hz: np.ndarray
    modes: np.ndarray
    residuals: np.ndarray
    iterations: int
    converged: int
    block: int
    precond: int


@dataclass
class AdjointResult:
    """What AdjointStep returns: the cotangents of the inputs of the step just solved.  f_ext, v_prev, x_prev [N, 3];
    lam_in, targets [n_constraints] (targets: of the fixed nodes in the order 3 slot + component, or the right-hand side
    of the CSR rows); gravity [3]; per_material [n_mat, P + 1] in the model's natural parameters -- SVK (lambda, mu),
    Mooney-Rivlin (mu10, mu01, kappa) -- then the density; per_element [E, P + 1] or None; iterations and rel_res of the
    linear solve."""
    f_ext: np.ndarray
    v_prev: np.ndarray
    x_prev: np.ndarray
    lam_in: np.ndarray
    targets: np.ndarray
    gravity: np.ndarray
    per_material: np.ndarray
    per_element: object
    iterations: int
    rel_res: float
    X_bar: object = None    # [N, 3] cotangent of the reference coordinates (AdjointStep(want_shape=True))


MODAL_DEFAULT_SHIFT = (2.0 * np.pi * 1.0) ** 2   # (2 pi 1 Hz)^2


class SyncedNewtonSolver:
    def __init__(self, data, n_constraints):
        self._lib = load_library()
        self._data = data  # the data object must outlive the solver (SyncedNewton.cuh:37-46)
        self.n_coef = data.get_n_coef()
        self.n_constraints = int(n_constraints)
        self._h = C.c_void_p()
        check(self._lib.tlfea_newton_create(data._h, self.n_constraints, C.byref(self._h)))
        self._cb = None

    def __del__(self):
        try:
            if self._h:
                self._lib.tlfea_newton_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Setup(self):
        check(self._lib.tlfea_newton_setup(self._h))

    def SetParameters(self, params):
        p = NewtonParams(params.inner_atol, params.inner_rtol, params.outer_tol, params.rho, params.max_outer,
                         params.max_inner, params.time_step)
        check(self._lib.tlfea_newton_set_parameters(self._h, C.byref(p)))

    def SetLinSolveOpts(self, o):
        c = LinSolveOptsC(o.rel_tol, o.max_iter, o.check_every, o.cheb_degree, o.cheb_kappa, o.cheb_bits, o.precond,
                          o.method, o.on_unconverged)
        check(self._lib.tlfea_newton_set_linsolve_opts(self._h, C.byref(c)))

    def GetLinSolveInfo(self):
        """(polynomial degree, matrix bits of its steps, bits of its work vectors) the auto rules resolved to"""
        deg, bits, vbits = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.tlfea_newton_get_linsolve_info(self._h, C.byref(deg), C.byref(bits), C.byref(vbits)))
        return deg.value, bits.value, vbits.value

    def GetPreconditioner(self):
        """0 block-Jacobi, 1 Chebyshev polynomial, 2 two-level p-multigrid (what a solve would use now)"""
        return int(self._lib.tlfea_newton_get_precond(self._h))

    def Collectives(self):
        """all-reduce calls issued by the engine since the solver was built (torch.distributed callback or built-in RCCL)"""
        self._lib.tlfea_newton_collectives.restype = C.c_long
        return int(self._lib.tlfea_newton_collectives(self._h))

    def GetAssemblyMode(self):
        """1: tangent blocks + row-owner gather (two launches), 2: fused tangent + assembly, general form, 3: its
        affine-element form (straight-sided T10, St.Venant-Kirchhoff)"""
        return int(self._lib.tlfea_newton_get_assembly_mode(self._h))

    ASSEMBLY_FORM_KEYS = ("mode", "rolled", "tangent_wpb", "groups", "acc_max", "lds_bytes", "workgroups", "passes")

    def GetAssemblyForm(self):
        """dict of the launch an assembly would issue now: mode (1 two kernels, 2 fused general, 3 fused affine), rolled,
        tangent_wpb (two-kernel path), groups, acc_max (doubles), lds_bytes, workgroups, passes (test hook)"""
        out = (C.c_int * 8)()
        check(self._lib.tlfea_newton_get_assembly_form(self._h, out))
        return dict(zip(self.ASSEMBLY_FORM_KEYS, (int(v) for v in out)))

    def GetGradientForm(self):
        """1: mass CSR product inside grad_kernel (TLFEA_MASS=csr, ANCF), 2: element inertia rows + grad_light_kernel (test hook)"""
        return int(self._lib.tlfea_newton_get_gradient_form(self._h))

    def RetrievePmgLevel(self):
        """(par0, par1, c_off, c_cols, Hc_values): parent map of the fine nodes, coarse node adjacency and the Galerkin
        operator P^T H P of the current H in the DOF-level layout of H (test hook)."""
        nc, nnz = C.c_int(), C.c_int()
        check(self._lib.tlfea_newton_pmg_sizes(self._h, C.byref(nc), C.byref(nnz)))
        par0, par1 = np.zeros(self.n_coef, dtype=np.int32), np.zeros(self.n_coef, dtype=np.int32)
        c_off, c_cols = np.zeros(nc.value + 1, dtype=np.int32), np.zeros(nnz.value, dtype=np.int32)
        Hc = np.zeros(9 * nnz.value)
        check(self._lib.tlfea_newton_pmg_retrieve(self._h, ip(par0), ip(par1), ip(c_off), ip(c_cols), dp(Hc)))
        return par0, par1, c_off, c_cols, Hc

    def RetrievePmgLevelBuilt(self):
        """(Hc_values, form): the Galerkin operator as the last preconditioner set-up left it on the device, nothing
        recomputed, and the kernel that summed it (1 gather, 2 row kernel alone, 3 row kernel fused with the build of R).
        Call it before RetrievePmgLevel / RetrievePmgLevel3, which sum Hc again (test hook)."""
        nc, nnz, form = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.tlfea_newton_pmg_sizes(self._h, C.byref(nc), C.byref(nnz)))
        Hc = np.zeros(9 * nnz.value)
        check(self._lib.tlfea_newton_pmg_retrieve_built(self._h, dp(Hc), C.byref(form)))
        return Hc, form.value

    def GetSetupForm(self):
        """dict(records, h_assemblies, h_current): 1 if the last p-multigrid set-up ran on the image rows of R assembled from
        the element records (TLFEA_SETUP_RECORDS), assemblies of H since the solver was created, and whether the H on the
        device is the one of the last assembly"""
        out = (C.c_longlong * 3)()
        check(self._lib.tlfea_newton_get_setup_form(self._h, out))
        return dict(records=int(out[0]), h_assemblies=int(out[1]), h_current=bool(out[2]))

    def RetrieveBlockDiagonal(self):
        """[N, 3, 3]: the fine level's diagonal blocks as the last set-up (or assembly from the records) left them (test hook)"""
        D = np.zeros(9 * self.n_coef)
        check(self._lib.tlfea_newton_get_block_diagonal(self._h, dp(D)))
        return D.reshape(-1, 3, 3)

    def RetrieveSetupImage(self):
        """the image rows of R of the last assembly from the element records, row I in H's row layout [d][len][3] at
        9 off[I] of RetrieveRestrictOp (test hook)"""
        n = C.c_longlong()
        check(self._lib.tlfea_newton_get_setup_image(self._h, None, C.byref(n)))
        img = np.zeros(max(1, n.value))
        check(self._lib.tlfea_newton_get_setup_image(self._h, dp(img), C.byref(n)))
        return img[:n.value]

    def GetRestrictOpInfo(self):
        """dict(active, n_coarse, blocks, contributions, fine_blocks, fine_bits) of the restricted fine operator
        R = S_c P^T S_f^-1 Hs as the last preconditioner set-up left it (active 0: the cycle runs the fine residual pass)"""
        out = (C.c_int * 6)()
        check(self._lib.tlfea_newton_pmg_restrict_op_sizes(self._h, out))
        return dict(zip(("active", "n_coarse", "blocks", "contributions", "fine_blocks", "fine_bits"), list(out)))

    def GetC32Geometry(self, level):
        """dict(regime, lanes, threads, upfront, rows_per_group, grid, resident) of the last non-final polynomial step launched
        on level 0 (fine), 1 (vertex) or 2 (third level); regime 1 bandwidth, 2 latency, 3 one-round, -1 none yet; resident:
        the occupancy query's answer for the instantiation launched, in workgroups (test hook)"""
        out = (C.c_int * 7)()
        check(self._lib.tlfea_newton_get_c32_geometry(self._h, int(level), out))
        return dict(zip(("regime", "lanes", "threads", "upfront", "rows_per_group", "grid", "resident"), list(out)))

    DIRECT_INFO_KEYS = ("fronts", "levels", "top_depth", "L_total", "F_cap0", "F_cap1", "F_cap_work", "F_cap_stack", "m_max",
                        "k_max", "k_zero", "nodes", "panel", "update_inner", "update_trailing", "update_wide", "extend_add",
                        "push", "levels_one_wg", "levels_stepwise", "fwd_step", "bwd_step")

    def GetDirectInfo(self):
        """dict of the native sparse direct solve's plan facts (fronts, levels, top_depth, L_total, the four F_cap, m_max,
        k_max, k_zero, nodes) and of the kernel launches its last factorisation + solve issued (test hook)"""
        out = (C.c_longlong * 22)()
        check(self._lib.tlfea_newton_get_direct_info(self._h, out))
        return dict(zip(self.DIRECT_INFO_KEYS, (int(v) for v in out)))

    def GetDirectFronts(self):
        """(order[nodes], fronts[n, 7]): elimination order (new -> old node) and per front c0, c1, depth, parent, node rows,
        child 0, child 1 of the native sparse direct solve's plan, children before parents (test hook)"""
        info = self.GetDirectInfo()
        order, fr = np.zeros(info["nodes"], dtype=np.int32), np.zeros(7 * info["fronts"], dtype=np.int32)
        check(self._lib.tlfea_newton_get_direct_fronts(self._h, ip(order), ip(fr)))
        return order, fr.reshape(-1, 7)

    def RetrieveRestrictOp(self):
        """(off, cols, vals[blocks, 3, 3]): R as stored after the last set-up, fp32 widened to double (test hook)"""
        info = self.GetRestrictOpInfo()
        off, cols = np.zeros(info["n_coarse"] + 1, dtype=np.int32), np.zeros(max(1, info["blocks"]), dtype=np.int32)
        vals = np.zeros(9 * max(1, info["blocks"]))
        check(self._lib.tlfea_newton_pmg_restrict_op_retrieve(self._h, ip(off), ip(cols), dp(vals)))
        return off, cols[:info["blocks"]], vals[:9 * info["blocks"]].reshape(-1, 3, 3)

    def RetrieveFineCopy(self):
        """(off, cols, vals[blocks, 3, 3], sc_f[3N], sc_c[3Nc]): the fine level's stored copy S_f H S_f in the node-block
        CSR of H, fp16 / fp32 widened to double, and the scalings of both levels (test hook)"""
        info = self.GetRestrictOpInfo()
        off, cols = np.zeros(self.n_coef + 1, dtype=np.int32), np.zeros(info["fine_blocks"], dtype=np.int32)
        vals, sc_f, sc_c = np.zeros(9 * info["fine_blocks"]), np.zeros(3 * self.n_coef), np.zeros(3 * max(1, info["n_coarse"]))
        check(self._lib.tlfea_newton_pmg_fine_copy_retrieve(self._h, ip(off), ip(cols), dp(vals), dp(sc_f), dp(sc_c)))
        return off, cols, vals.reshape(-1, 3, 3), sc_f, sc_c[:3 * info["n_coarse"]]

    def GetPmgCycleInfo(self):
        """dict(levels, fine_terms, vertex_terms, vertex_degree, level3_degree, level3_nodes) of the cycle in use (levels 0:
        polynomial preconditioner)"""
        out = (C.c_int * 6)()
        check(self._lib.tlfea_newton_pmg_cycle_info(self._h, out))
        return dict(zip(("levels", "fine_terms", "vertex_terms", "vertex_degree", "level3_degree", "level3_nodes"), list(out)))

    def GetPolynomialInfo(self):
        """dict(degree, kappa, block) of the polynomial preconditioner in use; block 12 = ANCF node-block scaling"""
        out = (C.c_int * 3)()
        check(self._lib.tlfea_newton_polynomial_info(self._h, out))
        return dict(zip(("degree", "kappa", "block"), list(out)))

    def ApplyPreconditioner(self, r):
        """z = M^-1 r with the CG preconditioner of the current assembled H, set up from cold lambda_max estimates started
        at r (test hook).  r [3N], or a block [m, 3N]: the operator is then set up once, from r[0], and applied to every
        row -- one fixed operator for all of them.  The solver's warm state is left as it was."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.shape[-1] == 3 * self.n_coef and r.ndim in (1, 2)
        z = np.zeros_like(r)
        if r.ndim == 1:
            check(self._lib.tlfea_newton_apply_preconditioner(self._h, dp(r), dp(z)))
        else:
            check(self._lib.tlfea_newton_apply_preconditioner_block(self._h, r.shape[0], dp(r), dp(z)))
        return z

    def GetPreconditionerState(self):
        """dict of what the last set-up (a solve or ApplyPreconditioner) left on the device: the coefficient table `coef`
        (pairs (c1, c2) per step), its layout (ks, cf_resid, cf_restart, cf_beta, cf_coarse, cf_level3, ks2, kc, k3),
        precond / levels / degree / smoother / block / bits, the lambda_max estimates and lam_safety (test hook)."""
        io, do, coef = (C.c_int * 16)(), (C.c_double * 8)(), np.zeros(512)
        check(self._lib.tlfea_newton_preconditioner_state(self._h, io, do, dp(coef), coef.size))
        names = ("precond", "levels", "degree", "ks", "cf_resid", "cf_restart", "cf_beta", "cf_coarse", "cf_level3", "ks2",
                 "kc", "k3", "smoother", "n_coef", "block", "bits")
        out = dict(zip(names, list(io)))
        out.update(coef=coef[:out["n_coef"]].copy(), lam_max=do[0], lam_c=do[1], lam3=do[2], lam_safety=do[3],
                   hook_lam=(do[4], do[5], do[6]))
        return out

    CG_TRACE_FORM = ("fused", "lanes", "nt", "tiled", "xcd", "grid", "graphs", "spmv32", "replaced_mask", "update", "matfree",
                     "degree", "precond", "bits", "block12", "update_grid", "replace_lanes", "replace_grid", "replace_xcd",
                     "xcd_mode")

    def CGTrace(self, b, k):
        """The solver's own iterative solve of H x = b for exactly k <= 8 iterations with every iterate copied out (test
        hook).  Returns dict(x, r, z, p, q [k+1, 3N]; sums [k+1, 4] the device's totals of the slot arrays r.z (even / odd
        iterations), p.q, r.r; slots [k+1, 5, 512] the raw slot arrays; form: what ran, see tlfea_newton_cg_trace).  Record
        0 is the start, record j follows iteration j - 1; p and q are those of the iteration just run."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        n, k = 3 * self.n_coef, int(k)
        assert b.shape == (n,) and 1 <= k <= 8
        vecs, sums, slots = np.zeros((k + 1, 5, n)), np.zeros((k + 1, 4)), np.zeros((k + 1, 5, 512))
        form = np.zeros(24, dtype=np.int32)
        check(self._lib.tlfea_newton_cg_trace(self._h, dp(b), k, dp(vecs), dp(sums), dp(slots), ip(form)))
        out = {nm: vecs[:, j, :].copy() for j, nm in enumerate(("x", "r", "z", "p", "q"))}
        out.update(sums=sums, slots=slots, form=dict(zip(self.CG_TRACE_FORM, (int(v) for v in form))))
        return out

    def GetPmgLevel3Info(self):
        """(aggregates, 3x3 blocks, polynomial degree) of the third level, (0, 0, 0) when the cycle has two levels"""
        na, nnz, deg = C.c_int(), C.c_int(), C.c_int()
        check(self._lib.tlfea_newton_pmg3_sizes(self._h, C.byref(na), C.byref(nnz), C.byref(deg)))
        return na.value, nnz.value, deg.value

    def RetrievePmgLevel3(self):
        """(agg[Nc], rvec[Nc,3], active[Na], off3, cols3, H3_values): test hook for H3 = P2^T Hc P2"""
        nc, nnz = C.c_int(), C.c_int()
        check(self._lib.tlfea_newton_pmg_sizes(self._h, C.byref(nc), C.byref(nnz)))
        na, nnz3, _ = self.GetPmgLevel3Info()
        agg, rvec, active = np.zeros(nc.value, dtype=np.int32), np.zeros(3 * nc.value), np.zeros(na, dtype=np.int32)
        off3, cols3, H3 = np.zeros(2 * na + 1, dtype=np.int32), np.zeros(nnz3, dtype=np.int32), np.zeros(9 * nnz3)
        check(self._lib.tlfea_newton_pmg3_retrieve(self._h, ip(agg), dp(rvec), ip(active), ip(off3), ip(cols3), dp(H3)))
        return agg, rvec.reshape(-1, 3), active, off3, cols3, H3

    def AnalyzeHessianSparsity(self):
        check(self._lib.tlfea_newton_analyze_hessian_sparsity(self._h))

    def SetFixedSparsityPattern(self, fixed):
        check(self._lib.tlfea_newton_set_fixed_sparsity_pattern(self._h, int(bool(fixed))))

    def Solve(self):
        check(self._lib.tlfea_newton_solve(self._h))

    OneStepNewtonCuDSS = Solve  # reference name of the same step (SyncedNewton.cuh:345-349)

    def GetVelocityGuessDevicePtr(self):
        return self._lib.tlfea_newton_velocity_guess_device_ptr(self._h)

    def compute_l2_norm_cublas(self, d_vec, n_dofs):
        out = C.c_double()
        check(self._lib.tlfea_newton_l2_norm(self._h, C.c_void_p(d_vec), int(n_dofs), C.byref(out)))
        return out.value

    # ---- engine extras ------------------------------------------------------------------------
    def SetVerbose(self, v):
        check(self._lib.tlfea_newton_set_verbose(self._h, int(v)))

    def SetProfiling(self, on):
        check(self._lib.tlfea_newton_set_profiling(self._h, int(bool(on))))

    def RetrieveHessianCSRToCPU(self):
        nnz = C.c_int()
        check(self._lib.tlfea_newton_hessian_nnz(self._h, C.byref(nnz)))
        ro = np.zeros(3 * self.n_coef + 1, dtype=np.int32)
        ci = np.zeros(nnz.value, dtype=np.int32)
        val = np.zeros(nnz.value)
        check(self._lib.tlfea_newton_retrieve_hessian_csr(self._h, ip(ro), ip(ci), dp(val)))
        return ro, ci, val

    def EvalGradient(self):
        ng = C.c_double()
        check(self._lib.tlfea_newton_eval_gradient(self._h, C.byref(ng)))
        return ng.value

    def AssembleHessian(self):
        check(self._lib.tlfea_newton_assemble_hessian(self._h))

    def LinearSolve(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b)
        it, rel = C.c_int(), C.c_double()
        check(self._lib.tlfea_newton_linear_solve(self._h, dp(b), dp(x), C.byref(it), C.byref(rel)))
        return x, it.value, rel.value

    def ApplyHessian(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        check(self._lib.tlfea_newton_apply_hessian(self._h, dp(x), dp(y)))
        return y

    def ModalAnalysis(self, n_modes, shift=None, tol=1e-8, max_iter=500, block_extra=None, seed=0):
        """The n_modes lowest natural frequencies and mode shapes K phi = omega^2 M phi at the current positions (K the
        tangent stiffness, contact and constraint-penalty stiffness included; pinned coefficients eliminated), by LOBPCG on
        the device with the Newton solver's preconditioner.  shift (rad^2/s^2, default (2 pi 1 Hz)^2) makes a
        free body's pencil definite; keep it at or below the lowest omega^2 of interest -- any positive value gives the
        same modes, only the iteration count changes.  General linear constraints stay as the penalty H carries.  Raises
        TlfeaError (with the modes found so far attached as .partial) when fewer than n_modes converge in max_iter; the
        solver's state is unchanged either way."""
        n_modes = int(n_modes)
        o = ModalOptsC(n_modes, -1 if block_extra is None else int(block_extra),
                       MODAL_DEFAULT_SHIFT if shift is None else float(shift), float(tol), int(max_iter), int(seed))
        k = max(n_modes, 1)
        w2, modes, res = np.zeros(k), np.zeros((k, 3 * self.n_coef)), np.zeros(k)
        info = np.zeros(4, dtype=np.int32)
        rc = self._lib.tlfea_newton_modal_solve(self._h, C.byref(o), dp(w2), dp(modes), dp(res), ip(info))
        out = ModalResult(w2, np.sqrt(np.maximum(w2, 0.0)) / (2.0 * np.pi), modes.reshape(k, self.n_coef, 3), res,
                          int(info[0]), int(info[1]), int(info[2]), int(info[3]))
        if rc != 0:
            err = TlfeaError(self._lib.tlfea_last_error().decode())
            err.partial = out
            raise err
        return out

    def AdjointReady(self):
        """Raises TlfeaError with the reason when AdjointStep would refuse the solver's state now."""
        check(self._lib.tlfea_newton_adjoint_ready(self._h))

    def AdjointStep(self, xbar=None, vbar=None, lambar=None, per_element=False, v_prev=None, want_shape=False):
        """Adjoint of the implicit step just solved (Solve() with max_outer = 1): given the cotangents of its
        outputs x, v [3N or N x 3] and lambda_new [n_constraints] (None = zero), one solve with the step's Hessian gives
        the cotangents of f_ext, v_prev, x_prev, lambda, the constraint targets, the body acceleration and the material
        parameters.  v_prev: the velocity the step started from (default: the one the last Solve() started from); it
        enters the density slot only.  want_shape adds X_bar [N, 3], the cotangent of the reference coordinates of every
        node (refused with an obstacle or a face traction set).  The solver's state is left as it was."""
        n, nc = 3 * self.n_coef, int(self._lib.tlfea_newton_n_constraints(self._h))
        self.n_constraints = nc

        def arr(a, size, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
            if a.size != size:
                raise ValueError(f"AdjointStep: {name} needs {size} entries, got {a.size}")
            return a
        ins = [arr(xbar, n, "xbar"), arr(vbar, n, "vbar"), arr(lambar, nc, "lambar"), arr(v_prev, n, "v_prev")]
        n_mat, slots = self._data.MaterialSensitivityShape()
        outs = [np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(nc), np.zeros(nc), np.zeros(3), np.zeros((n_mat, slots)),
                np.zeros((self._data.n_elem, slots)) if per_element else None]
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
        cin, cout = AdjointInC(*[ptr(a) for a in ins]), AdjointOutC(*[ptr(a) for a in outs])
        it, rel = C.c_int(), C.c_double()
        N = self.n_coef
        X_bar = np.zeros((N, 3)) if want_shape else None
        if want_shape:
            check(self._lib.tlfea_newton_adjoint_step_shape(self._h, C.byref(cin), C.byref(cout), X_bar.ctypes.data,
                                                            C.byref(it), C.byref(rel)))
        else:
            check(self._lib.tlfea_newton_adjoint_step(self._h, C.byref(cin), C.byref(cout), C.byref(it), C.byref(rel)))
        return AdjointResult(outs[0].reshape(N, 3), outs[1].reshape(N, 3), outs[2].reshape(N, 3), outs[3], outs[4],
                             outs[5], outs[6], outs[7], it.value, rel.value, X_bar)

    def AdjointStepDevice(self, cin, cout, X_bar=None):
        """The same on device pointers (binding.AdjointInC / AdjointOutC filled with device addresses, 0 / None = absent):
        -> (iterations, rel_res).  X_bar: device address of [3N] doubles for the cotangent of the reference coordinates
        (None = not wanted).  differentiable.ImplicitStep calls this with torch tensors."""
        it, rel = C.c_int(), C.c_double()
        if X_bar is None:
            check(self._lib.tlfea_newton_adjoint_step_device(self._h, C.byref(cin), C.byref(cout), C.byref(it), C.byref(rel)))
        else:
            check(self._lib.tlfea_newton_adjoint_step_shape_device(self._h, C.byref(cin), C.byref(cout), C.c_void_p(X_bar),
                                                                   C.byref(it), C.byref(rel)))
        return it.value, rel.value

    # -- the same on ANCF beam and shell objects (DESIGN 3j'); AdjointStep stays T10-only and keeps refusing -----------------
    def ANCFAdjointReady(self):
        """Raises TlfeaError with the reason when ANCFAdjointStep would refuse the solver's state now."""
        check(self._lib.tlfea_newton_ancf_adjoint_ready(self._h))

    def ANCFAdjointStep(self, x_bar=None, v_bar=None, lam_bar=None, v_prev=None, want=("per_material",)):
        """AdjointStep on an ANCF object: every vector runs over the n_coef coefficient vectors; the body acceleration
        acts on the position coefficients (index % 4 == 0), so `gravity` sums M w over those; targets are those of the
        fixed coefficients (3 slot + component) or the right-hand side of the CSR rows.  `want`: which of "per_material"
        [1, P + 1] (stiffness slots, then the density: -(M w).u / rho0) and "per_element" [E, P] (stiffness slots only)
        to compute; the vector outputs always come.  The solver's state is left as it was."""
        n, nc = 3 * self.n_coef, int(self._lib.tlfea_newton_n_constraints(self._h))
        self.n_constraints = nc
        unknown = set(want) - {"per_material", "per_element"}
        if unknown:
            raise ValueError(f"ANCFAdjointStep: want holds {sorted(unknown)}; it takes 'per_material' and 'per_element'")

        def arr(a, size, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
            if a.size != size:
                raise ValueError(f"ANCFAdjointStep: {name} needs {size} entries, got {a.size}")
            return a
        ins = [arr(x_bar, n, "x_bar"), arr(v_bar, n, "v_bar"), arr(lam_bar, nc, "lam_bar"), arr(v_prev, n, "v_prev")]
        n_mat, slots = self._data.ANCFMaterialSensitivityShape()
        outs = [np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(nc), np.zeros(nc), np.zeros(3),
                np.zeros((n_mat, slots)) if "per_material" in want else None,
                np.zeros((self._data.n_elem, slots - 1)) if "per_element" in want else None]
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
        cin, cout = AdjointInC(*[ptr(a) for a in ins]), AdjointOutC(*[ptr(a) for a in outs])
        it, rel = C.c_int(), C.c_double()
        check(self._lib.tlfea_newton_ancf_adjoint_step(self._h, C.byref(cin), C.byref(cout), C.byref(it), C.byref(rel)))
        N = self.n_coef
        return AdjointResult(outs[0].reshape(N, 3), outs[1].reshape(N, 3), outs[2].reshape(N, 3), outs[3], outs[4],
                             outs[5], outs[6], outs[7], it.value, rel.value)

    def ANCFAdjointStepDevice(self, cin, cout):
        """The same on device pointers (binding.AdjointInC / AdjointOutC filled with device addresses, 0 / None = absent):
        -> (iterations, rel_res).  differentiable.ImplicitStep calls this with torch tensors."""
        it, rel = C.c_int(), C.c_double()
        check(self._lib.tlfea_newton_ancf_adjoint_step_device(self._h, C.byref(cin), C.byref(cout), C.byref(it), C.byref(rel)))
        return it.value, rel.value

    def ModalApplyBlock(self, X, which=0, apply_mask=False):
        """Y = H X (which 0) or (M (x) I3) X (which 1) for a block X [3N, m], m <= 32, with the current H (test hook)"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert X.ndim == 2 and X.shape[0] == 3 * self.n_coef
        Y = np.zeros_like(X)
        check(self._lib.tlfea_newton_modal_apply_block(self._h, int(which), X.shape[1], dp(X), dp(Y), int(bool(apply_mask))))
        return Y

    def ModalGram(self, X, Y):
        """G = X^T Y for blocks [3N, p], [3N, q], p, q <= 96, by the modal solve's deterministic Gram kernels (test hook)"""
        X, Y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(Y, dtype=np.float64)
        assert X.ndim == 2 and Y.ndim == 2 and X.shape[0] == Y.shape[0] == 3 * self.n_coef
        G = np.zeros((X.shape[1], Y.shape[1]))
        check(self._lib.tlfea_newton_modal_gram(self._h, X.shape[1], Y.shape[1], dp(X), dp(Y), dp(G)))
        return G

    def ModalTimeSpmm(self, m, reps=20):
        """mean ms of one block product Y = H X with m columns over `reps` back-to-back launches (hipEvents)"""
        out = C.c_double()
        check(self._lib.tlfea_newton_modal_time_spmm(self._h, int(m), int(reps), C.byref(out)))
        return out.value

    def ApplyHessianMatfree(self, x):
        """y = H x from the matrix-free pair of the CG iteration (raises where it is not eligible)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        check(self._lib.tlfea_newton_apply_hessian_matfree(self._h, dp(x), dp(y)))
        return y

    def GetSpmvMode(self):
        """product of the last solve's CG iterations: 0 CSR kernel, 1 matrix-free pair"""
        return int(self._lib.tlfea_newton_get_spmv_mode(self._h))

    def GetFineSmoother(self):
        """fine smoother the last preconditioner set-up chose: 0 stream of the low-precision copy, 1 passes from the
        element records (DESIGN 3g')"""
        return int(self._lib.tlfea_newton_get_fine_smoother(self._h))

    def GetFineCopyState(self):
        """(bits, current, conversions) of the fine level's low-precision copy: bits allocated (0: none), whether it is that
        of the last set-up's H, fine-level conversions since creation.  A set-up that takes the fine smoother from the
        element records converts nothing; read-backs and timings convert on demand (test hook)"""
        out = (C.c_int * 3)()
        check(self._lib.tlfea_newton_get_fine_copy_state(self._h, out))
        return tuple(int(v) for v in out)

    def FineSmootherPass(self, d, res, z, r, coef, zw=0.0, last=False):
        """one fine smoother pass from the element records with the set-up the last ApplyPreconditioner left (test hook):
        (d', z^', res^') as float32, or with last (d', z = S z^' in float64, the 512 r.z slots)"""
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        n = 3 * self.n_coef
        d, res, z = (np.ascontiguousarray(a, dtype=np.float32) for a in (d, res, z))
        r = np.ascontiguousarray(r, dtype=np.float64)
        cf = np.ascontiguousarray(coef, dtype=np.float64)
        assert d.shape == res.shape == z.shape == r.shape == (n,) and cf.shape == (2,)
        d_o, z_o, r_o = (np.zeros(n, dtype=np.float32) for _ in range(3))
        z64, slots = np.zeros(n), np.zeros(512)
        check(self._lib.tlfea_newton_fine_smoother_pass(self._h, fp(d), fp(res), fp(z), dp(r), dp(cf), float(zw), int(bool(last)),
                                                        fp(d_o), fp(z_o), fp(r_o), dp(z64), dp(slots)))
        return (d_o, z64, slots) if last else (d_o, z_o, r_o)

    def GetLambdaMax(self):
        """(fine, vertex, level3, matfree): the last lambda_max estimates of the three levels (0 where a level does not
        exist) and whether the last fine estimate ran its products through the matrix-free pair"""
        out = np.zeros(4)
        check(self._lib.tlfea_newton_get_lambda_max(self._h, dp(out)))
        return float(out[0]), float(out[1]), float(out[2]), bool(out[3] != 0.0)

    def GetMatfreeRows(self):
        """(form, rows, ratio) of the matrix-free pair's row buffer: form 1 = summed per wavefront and node, 0 = one row per
        (element, local node), -1 = the pair has not run; ratio = 10 E / rows"""
        rows, ratio = C.c_longlong(), C.c_double()
        form = int(self._lib.tlfea_newton_get_matfree_rows(self._h, C.byref(rows), C.byref(ratio)))
        return form, int(rows.value), float(ratio.value)

    def GetMatfreeRecords(self, which, single=False):
        """(points, values): element records of the matrix-free passes (test hook).  which 0 / 1: the element-major g
        [E, 16] / F [E, 5, 10] in float64; 2 / 3: the packed g / F (csrc/matfree_records.h) of the fp64 product, or with
        single of the float smoother passes, as a flat array.  points = stored points of the packed F of that type"""
        n, pts = C.c_longlong(), C.c_int()
        f = self._lib.tlfea_newton_get_matfree_records
        check(f(self._h, int(bool(single)), int(which), None, C.byref(n), C.byref(pts)))
        out = np.zeros(n.value, dtype=np.float32 if single and which >= 2 else np.float64)
        check(f(self._h, int(bool(single)), int(which), out.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(pts)))
        pts = int(pts.value)
        if which == 0:
            out = out.reshape(-1, 16)
        elif which == 1:
            out = out.reshape(-1, 5, 10)
        return pts, out

    def NewtonIteration(self):
        ng, it = C.c_double(), C.c_int()
        check(self._lib.tlfea_newton_iteration(self._h, C.byref(ng), C.byref(it)))
        return ng.value, it.value

    def RetrieveGradientToCPU(self):
        g = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_newton_retrieve_gradient(self._h, dp(g)))
        return g

    def RetrieveVelocityToCPU(self):
        v = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_newton_retrieve_velocity(self._h, dp(v)))
        return v

    def SetVelocity(self, v, v_prev=None):
        v = np.ascontiguousarray(v, dtype=np.float64)
        vp = np.ascontiguousarray(v_prev, dtype=np.float64) if v_prev is not None else None
        check(self._lib.tlfea_newton_set_velocity(self._h, dp(v), dp(vp)))

    def SetLambda(self, lam):
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        assert lam.size == self.n_constraints
        check(self._lib.tlfea_newton_set_lambda(self._h, dp(lam)))

    def RetrieveLambdaToCPU(self):
        self.n_constraints = int(self._lib.tlfea_newton_n_constraints(self._h))   # follows UpdateNodalFixed
        lam = np.zeros(self.n_constraints)
        check(self._lib.tlfea_newton_retrieve_lambda(self._h, dp(lam)))
        return lam

    def GetStats(self):
        st = np.zeros(6)
        check(self._lib.tlfea_newton_get_stats(self._h, dp(st)))
        return dict(outer=int(st[0]), newton=int(st[1]), norm_g=st[2], norm_c=st[3], pcg_iters=int(st[4]), ms=st[5])

    def GetLinSolveStatus(self):
        """Linear solves since the last Solve() / NewtonIteration() began: relative residual and tolerance flag of the
        last one, worst relative residual, and whether all of them met rel_tol."""
        st = np.zeros(4)
        check(self._lib.tlfea_newton_get_linsolve_status(self._h, dp(st)))
        return dict(rel_res=st[0], converged=bool(st[1]), worst_rel_res=st[2], all_converged=bool(st[3]))

    STAGES = ["residual", "grad", "tangent_blocks", "assemble_rows", "pcg", "update", "spmv", "_"]

    def GetStageMs(self, reset=False):
        """-> {stage: (total_ms, launches)} measured with hipEvents on the launch stream (profiling mode)."""
        ms, cnt = np.zeros(8), np.zeros(8)
        check(self._lib.tlfea_newton_get_stage_ms(self._h, dp(ms), dp(cnt), int(reset)))
        return {k: (ms[i], int(cnt[i])) for i, k in enumerate(self.STAGES) if k != "_"}

    def TimeKernels(self, reps=20):
        """-> {kernel: mean ms} over `reps` back-to-back launches each (hipEvents on the launch stream)."""
        out = np.zeros(7)
        check(self._lib.tlfea_newton_time_kernels(self._h, int(reps), dp(out)))
        return dict(zip(["residual", "tangent_blocks", "assemble_rows", "spmv", "cheb_step", "cheb_step_coarse",
                         "cheb_step_cycle"], out.tolist()))

    def GetPmgInfo(self):
        """(coarse nodes, coarse 3x3 blocks, coarse polynomial degree) of the p-multigrid level, or None"""
        if self.GetPreconditioner() != 2:
            return None
        nc, nnz = C.c_int(), C.c_int()
        check(self._lib.tlfea_newton_pmg_sizes(self._h, C.byref(nc), C.byref(nnz)))
        return nc.value, nnz.value, int(self._lib.tlfea_newton_pmg_coarse_degree(self._h))

    def BeginStep(self):
        check(self._lib.tlfea_newton_begin_step(self._h))

    def SetInterface(self, iface_nodes, iface_slots, n_global_iface, node_weight, allreduce, sync_before_callback=1):
        """allreduce(ptr:int, n:int) sums a device buffer of n doubles over ranks in place (see partition.py)."""
        nodes = np.ascontiguousarray(iface_nodes, dtype=np.int32)
        slots = np.ascontiguousarray(iface_slots, dtype=np.int32)
        w = np.ascontiguousarray(node_weight, dtype=np.float64)
        assert w.size == self.n_coef and nodes.size == slots.size

        def _cb(_user, ptr, n):
            try:
                allreduce(ptr, n)
                return 0
            except Exception as exc:  # pragma: no cover
                print("allreduce callback failed:", repr(exc), flush=True)
                return 1

        self.n_collectives = 0

        def _cb_counted(user, ptr, n):
            self.n_collectives += 1
            return _cb(user, ptr, n)

        self._cb = ALLREDUCE_FN(_cb_counted)
        check(self._lib.tlfea_newton_set_interface(self._h, ip(nodes), ip(slots), int(nodes.size),
                                                   int(n_global_iface), dp(w), self._cb, None,
                                                   int(sync_before_callback)))

    def SetInterfaceRccl(self, iface_nodes, iface_slots, n_global_iface, node_weight, comm):
        """The same interface with the library's built-in RCCL all-reduce (tlfea_rccl_allreduce_fn): the collective is
        enqueued from C++ on the solver's launch stream, no Python in the loop.  comm: handle from
        partition.rccl_communicator()."""
        nodes = np.ascontiguousarray(iface_nodes, dtype=np.int32)
        slots = np.ascontiguousarray(iface_slots, dtype=np.int32)
        w = np.ascontiguousarray(node_weight, dtype=np.float64)
        assert w.size == self.n_coef and nodes.size == slots.size
        self._lib.tlfea_rccl_allreduce_fn.restype = C.c_void_p
        fn = C.cast(self._lib.tlfea_rccl_allreduce_fn(), ALLREDUCE_FN)
        self.n_collectives = -1   # not counted on this path
        self._cb = fn
        check(self._lib.tlfea_newton_set_interface(self._h, ip(nodes), ip(slots), int(nodes.size),
                                                   int(n_global_iface), dp(w), fn, comm, 0))

    def SetHalo(self, part, allreduce=None, exchange=None, sync_before_callback=1, rccl_comm=None):
        """Overlapping partition (tlfea_newton_set_halo): `part` is a partition.HaloPartition built on the mesh this
        solver's data object holds.  Either Python callbacks -- allreduce(ptr, n) sums n device doubles over ranks in
        place, exchange(send_ptr, recv_ptr, peers, send_off, recv_off) moves byte ranges neighbour to neighbour -- or
        rccl_comm: the library's built-in RCCL exchange on a communicator of partition.rccl_communicator()."""
        from .binding import HALO_EXCHANGE_FN, HaloListsC
        assert len(part.layer) == self.n_coef
        P = len(part.peers)
        peers = np.ascontiguousarray(part.peers, dtype=np.int32)
        cat = lambda arrs: (np.ascontiguousarray(np.concatenate(arrs), dtype=np.int32) if arrs else np.zeros(0, np.int32))  # noqa: E731
        off = lambda arrs: np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(a) for a in arrs])]), dtype=np.int32)  # noqa: E731
        so, ro = off(part.send), off(part.recv)
        sn, sl, rn = cat(part.send), cat(part.send_layer), cat(part.recv)
        layer = np.ascontiguousarray(part.layer, dtype=np.int32)
        lists = HaloListsC(P, ip(peers), ip(so), ip(sn), ip(sl), ip(ro), ip(rn), int(part.rank), int(part.world))
        self._halo_keep = (peers, so, ro, sn, sl, rn, layer, lists)
        if rccl_comm is not None:
            self._lib.tlfea_rccl_allreduce_fn.restype = C.c_void_p
            self._lib.tlfea_rccl_halo_exchange_fn.restype = C.c_void_p
            ar = C.cast(self._lib.tlfea_rccl_allreduce_fn(), ALLREDUCE_FN)
            ex = C.cast(self._lib.tlfea_rccl_halo_exchange_fn(), HALO_EXCHANGE_FN)
            self._cb = (ar, ex)
            check(self._lib.tlfea_newton_set_halo(self._h, ip(layer), int(part.depth), C.byref(lists), ar, ex, rccl_comm, 0))
            return

        def _ar(_user, ptr, n):
            try:
                allreduce(ptr, n)
                return 0
            except Exception as exc:  # pragma: no cover
                print("allreduce callback failed:", repr(exc), flush=True)
                return 1

        def _ex(_user, sp, rp, n_peers, peers_p, so_p, ro_p):
            try:
                exchange(sp, rp, [peers_p[k] for k in range(n_peers)], [so_p[k] for k in range(n_peers + 1)],
                         [ro_p[k] for k in range(n_peers + 1)])
                return 0
            except Exception as exc:  # pragma: no cover
                print("halo exchange callback failed:", repr(exc), flush=True)
                return 1

        self._cb = (ALLREDUCE_FN(_ar), HALO_EXCHANGE_FN(_ex))
        check(self._lib.tlfea_newton_set_halo(self._h, ip(layer), int(part.depth), C.byref(lists), self._cb[0], self._cb[1],
                                              None, int(sync_before_callback)))

    def GetCommStats(self):
        out = np.zeros(8)
        check(self._lib.tlfea_newton_get_comm_stats(self._h, dp(out)))
        return dict(exchanges=int(out[0]), allreduces=int(out[1]), bytes_exchanged=float(out[2]), bytes_allreduced=float(out[3]),
                    comm_ms=float(out[4]), cg_iterations=int(out[5]), exchanges_in_cg=int(out[6]), allreduces_in_cg=int(out[7]))

    def SetInterfaceOwners(self, node_owned):
        """node_owned[n_coef] = 1 where this rank owns the node (one owner per replicated node over all ranks):
        switches the polynomial preconditioner to its rank-local form (see tlfea_c.h)."""
        own = np.ascontiguousarray(node_owned, dtype=np.int32)
        assert own.size == self.n_coef
        check(self._lib.tlfea_newton_set_interface_owners(self._h, ip(own)))


@dataclass
class SyncedAdamWNocoopParams:
    """SyncedAdamWParams, field order of SyncedAdamW.cuh:27-34 (drivers: test_ancf3243.cc:374-376)."""
    lr: float = 2e-4
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    weight_decay: float = 1e-4
    lr_decay: float = 0.998
    inner_tol: float = 1e-1
    outer_tol: float = 1e-6
    rho: float = 1e14
    max_outer: int = 5
    max_inner: int = 500
    time_step: float = 1e-3
    convergence_check_interval: int = 10
    inner_rtol: float = 0.0


class SyncedAdamWNocoopSolver:
    """SyncedAdamWNocoopSolver (SyncedAdamWNocoop.cuh:22-198): first-order ALM solver on the element kernels."""

    def __init__(self, data, n_constraints):
        self._lib = load_library()
        self._data = data
        self.n_coef = data.get_n_coef()
        self.n_constraints = int(n_constraints)
        self._h = C.c_void_p()
        check(self._lib.tlfea_adamw_create(data._h, self.n_constraints, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.tlfea_adamw_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Setup(self):
        check(self._lib.tlfea_adamw_setup(self._h))

    def SetParameters(self, p):
        c = AdamWParamsC(p.lr, p.beta1, p.beta2, p.eps, p.weight_decay, p.lr_decay, p.inner_tol, p.outer_tol, p.rho,
                         p.max_outer, p.max_inner, p.time_step, p.convergence_check_interval, p.inner_rtol)
        check(self._lib.tlfea_adamw_set_parameters(self._h, C.byref(c)))

    def Solve(self):
        check(self._lib.tlfea_adamw_solve(self._h))

    OneStepAdamWNocoop = Solve

    def SetVerbose(self, v):
        check(self._lib.tlfea_adamw_set_verbose(self._h, int(v)))

    def GetVelocityGuessDevicePtr(self):
        self._lib.tlfea_adamw_velocity_guess_device_ptr.restype = C.c_void_p
        return self._lib.tlfea_adamw_velocity_guess_device_ptr(self._h)

    def RetrieveVelocityToCPU(self):
        v = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_adamw_retrieve_velocity(self._h, dp(v)))
        return v

    def RetrieveLambdaToCPU(self):
        lam = np.zeros(self.n_constraints)
        check(self._lib.tlfea_adamw_retrieve_lambda(self._h, dp(lam)))
        return lam

    def GetStats(self):
        st = np.zeros(6)
        check(self._lib.tlfea_adamw_get_stats(self._h, dp(st)))
        return dict(outer=int(st[0]), inner=int(st[1]), norm_g=st[2], norm_c=st[3], inner_flag=int(st[4]), ms=st[5])


class SyncedAdamWSolver(SyncedAdamWNocoopSolver):
    """SyncedAdamWSolver (SyncedAdamW.cuh, SyncedAdamW.cu:96-445): the cooperative-kernel sibling of the same solver; as
    written there the inner-converged flag is cleared once per Solve(), the multipliers get rho*dt*c once and the outer
    loop stops on ||c|| < outer_tol alone."""

    def __init__(self, data, n_constraints):
        super().__init__(data, n_constraints)
        check(self._lib.tlfea_adamw_set_cooperative_semantics(self._h, 1))

    OneStepAdamW = SyncedAdamWNocoopSolver.Solve


SyncedAdamWParams = SyncedAdamWNocoopParams


@dataclass
class SyncedNesterovParams:
    """SyncedNesterovParams (SyncedNesterov.cuh:26-30; driver values test_ancf3243.cc:351-352)."""
    alpha: float = 1e-8
    rho: float = 1e14
    inner_tol: float = 1e-6
    outer_tol: float = 1e-6
    max_outer: int = 5
    max_inner: int = 200
    time_step: float = 1e-3


class SyncedNesterovSolver:
    """SyncedNesterovSolver (SyncedNesterov.cuh:32-260): accelerated-gradient ALM solver on the element kernels."""

    def __init__(self, data, n_constraints):
        self._lib = load_library()
        self._data = data
        self.n_coef = data.get_n_coef()
        self.n_constraints = int(n_constraints)
        self._h = C.c_void_p()
        check(self._lib.tlfea_nesterov_create(data._h, self.n_constraints, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.tlfea_nesterov_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Setup(self):
        check(self._lib.tlfea_nesterov_setup(self._h))

    def SetParameters(self, p):
        c = NesterovParamsC(p.alpha, p.rho, p.inner_tol, p.outer_tol, p.max_outer, p.max_inner, p.time_step)
        check(self._lib.tlfea_nesterov_set_parameters(self._h, C.byref(c)))

    def Solve(self):
        check(self._lib.tlfea_nesterov_solve(self._h))

    OneStepNesterov = Solve

    def SetVerbose(self, v):
        check(self._lib.tlfea_nesterov_set_verbose(self._h, int(v)))

    def GetVelocityGuessDevicePtr(self):
        return self._lib.tlfea_nesterov_velocity_guess_device_ptr(self._h)

    def RetrieveVelocityToCPU(self):
        v = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_nesterov_retrieve_velocity(self._h, dp(v)))
        return v

    def RetrieveLambdaToCPU(self):
        lam = np.zeros(self.n_constraints)
        check(self._lib.tlfea_nesterov_retrieve_lambda(self._h, dp(lam)))
        return lam

    def GetStats(self):
        st = np.zeros(6)
        check(self._lib.tlfea_nesterov_get_stats(self._h, dp(st)))
        return dict(outer=int(st[0]), inner=int(st[1]), norm_g=st[2], norm_c=st[3], inner_flag=int(st[4]), ms=st[5])


@dataclass
class SyncedVBDParams:
    """SyncedVBDParams (SyncedVBD.cuh:13-21; driver values test_feat10_resolution.cc:379-380 with omega 1.8)."""
    inner_tol: float = 1e-4
    inner_rtol: float = 1e-4
    outer_tol: float = 1e-4
    rho: float = 1e14
    max_outer: int = 5
    max_inner: int = 500
    time_step: float = 1e-3
    omega: float = 1.0
    hess_eps: float = 1e-12
    convergence_check_interval: int = 25
    color_group_size: int = 1


class SyncedVBDSolver:
    """SyncedVBDSolver (SyncedVBD.cuh:23-330): vertex block descent -- coloured per-node 3x3 Newton sweeps."""

    def __init__(self, data, n_constraints):
        self._lib = load_library()
        self._data = data
        self.n_coef = data.get_n_coef()
        self.n_constraints = int(n_constraints)
        self._h = C.c_void_p()
        check(self._lib.tlfea_vbd_create(data._h, self.n_constraints, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.tlfea_vbd_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Setup(self):
        check(self._lib.tlfea_vbd_setup(self._h))

    def SetParameters(self, p):
        c = VbdParamsC(p.inner_tol, p.inner_rtol, p.outer_tol, p.rho, p.max_outer, p.max_inner, p.time_step, p.omega,
                       p.hess_eps, p.convergence_check_interval, p.color_group_size)
        check(self._lib.tlfea_vbd_set_parameters(self._h, C.byref(c)))

    def InitializeColoring(self):
        check(self._lib.tlfea_vbd_initialize_coloring(self._h))

    def InitializeMassDiagBlocks(self):
        check(self._lib.tlfea_vbd_initialize_mass_diag_blocks(self._h))

    def InitializeFixedMap(self):
        check(self._lib.tlfea_vbd_initialize_fixed_map(self._h))

    def Solve(self):
        check(self._lib.tlfea_vbd_solve(self._h))

    OneStepVBD = Solve

    def SetVerbose(self, v):
        check(self._lib.tlfea_vbd_set_verbose(self._h, int(v)))

    def GetColoring(self):
        """colors[N], color_offsets, color_nodes, group_offsets, group_colors of InitializeColoring"""
        nc, ng = C.c_int(), C.c_int()
        check(self._lib.tlfea_vbd_coloring_sizes(self._h, C.byref(nc), C.byref(ng)))
        out = dict(n_colors=nc.value, n_groups=ng.value, colors=np.zeros(self.n_coef, dtype=np.int32),
                   color_offsets=np.zeros(nc.value + 1, dtype=np.int32), color_nodes=np.zeros(self.n_coef, dtype=np.int32),
                   group_offsets=np.zeros(ng.value + 1, dtype=np.int32), group_colors=np.zeros(nc.value, dtype=np.int32))
        check(self._lib.tlfea_vbd_retrieve_coloring(self._h, ip(out["colors"]), ip(out["color_offsets"]),
                                                    ip(out["color_nodes"]), ip(out["group_offsets"]), ip(out["group_colors"])))
        return out

    def GetVelocityGuessDevicePtr(self):
        return self._lib.tlfea_vbd_velocity_guess_device_ptr(self._h)

    def RetrieveVelocityToCPU(self):
        v = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_vbd_retrieve_velocity(self._h, dp(v)))
        return v

    def RetrieveLambdaToCPU(self):
        lam = np.zeros(self.n_constraints)
        check(self._lib.tlfea_vbd_retrieve_lambda(self._h, dp(lam)))
        return lam

    def GetStats(self):
        st = np.zeros(6)
        check(self._lib.tlfea_vbd_get_stats(self._h, dp(st)))
        return dict(outer=int(st[0]), sweeps=int(st[1]), norm_g=st[2], norm_c=st[3], ms=st[5])
