"""Worker of tests/test_gpu_setup_kernels.py.  The library reads its TLFEA_* switches once per process, so every (mesh,
switches) pair runs as `python -m tests.setup_kernels_worker <full|solve> <mesh>` in a fresh child (the caller sets
TLFEA_PMG_LEVELS=3, TLFEA_SPMV_MATFREE=1 and TLFEA_LMAX_MATFREE).  Prints one JSON line last.

    full   Hc, H3 and R of the assembled H against their NumPy restatements, two builds each, then the solves
    solve  the solves only: a cold lambda_max estimate in the first, warm ones in the two that follow"""
import json
import sys

import numpy as np
import scipy.sparse as sp

from tests import galerkin_np as gn
from tests import precond_worker as pw
from tests import restricted_op_np as rn
from tests.helpers import tl

REL_TOL = 1e-12


def level3_reference(c_off, c_cols, Hc, agg, rvec, active, na):
    """P2^T Hc P2 with u_i = t_A + w_A x r_i (W_i0 = I, W_i1 = -[r_i]x) and the identity blocks of unusable aggregates"""
    nc = len(c_off) - 1
    rows, cols, vals = [], [], []
    for i in range(nc):
        A, r = agg[i], rvec[i]
        S = -np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        for a in range(3):
            rows.append(3 * i + a); cols.append(6 * A + a); vals.append(1.0)
            for b in range(3):
                if S[a, b] != 0.0:
                    rows.append(3 * i + a); cols.append(6 * A + 3 + b); vals.append(S[a, b])
    P2 = sp.csr_matrix((vals, (rows, cols)), shape=(3 * nc, 6 * na))
    ref = (P2.T @ gn.dof_csr(c_off, c_cols, Hc) @ P2).toarray()
    for A in np.where(active <= 0)[0]:
        ref[6 * A + 3:6 * A + 6, 6 * A + 3:6 * A + 6] = np.eye(3)
    for A in np.where(active < 0)[0]:
        ref[6 * A:6 * A + 3, 6 * A:6 * A + 3] = np.eye(3)
    return ref


def galerkin_checks(s, out):
    n = 3 * s.n_coef
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    H = sp.csr_matrix((val, ci, ro), shape=(n, n))
    out["H_asym"] = float(abs(H - H.T).max() / abs(H).max())
    par0, par1, c_off, c_cols, Hc = s.RetrievePmgLevel()
    Hc2 = s.RetrievePmgLevel()[4]
    nc = len(c_off) - 1
    P = gn.prolongation(par0, par1, nc)
    ref = (P.T @ H @ P).tocsr()
    dev = gn.dof_csr(c_off, c_cols, Hc)
    out["hc_relerr"] = float(abs(dev - ref).max() / abs(ref).max())
    asym = (dev - dev.T).tocoo()
    off_diag = asym.row // 3 != asym.col // 3
    out["hc_asym_offdiag"] = float(np.abs(asym.data[off_diag]).max(initial=0.0))
    out["hc_asym_diag_rel"] = float(np.abs(asym.data[~off_diag]).max(initial=0.0) / abs(ref).max())
    out["hc_bitwise_rebuild"] = bool(np.array_equal(Hc, Hc2))
    out["n_vertex"], out["hc_blocks"] = nc, int(len(c_cols))
    # third level
    na, nnz3, _ = s.GetPmgLevel3Info()
    out["n_aggregates"] = int(na)
    if na > 0:
        agg, rvec, active, off3, cols3, H3 = s.RetrievePmgLevel3()
        H3b = s.RetrievePmgLevel3()[5]
        ref3 = level3_reference(c_off, c_cols, Hc, agg, rvec, active, na)
        dev3 = gn.dof_csr(off3, cols3, H3).toarray()
        out["h3_relerr"] = float(np.abs(dev3 - ref3).max() / np.abs(ref3).max())
        out["h3_bitwise_rebuild"] = bool(np.array_equal(H3, H3b))
        # contributions per aggregate pair, from the retrieved aggregates and the vertex pattern: the lists of the kernel
        bi = np.repeat(np.arange(nc), np.diff(c_off))
        pairs = np.unique(agg[bi].astype(np.int64) * na + agg[c_cols], return_counts=True)[1]
        out["pair_contributions"] = [int(pairs.min()), int(pairs.max())]
        out["n_pairs"] = int(len(pairs))


def restrict_op_checks(s, out):
    r = np.random.default_rng(11).normal(size=3 * s.n_coef)
    s.ApplyPreconditioner(r)
    info = s.GetRestrictOpInfo()
    out["rop_info"] = info
    if info["active"] != 1:
        return
    off, cols, vals = s.RetrieveRestrictOp()
    f_off, f_cols, f_vals, sc_f, sc_c = s.RetrieveFineCopy()
    par0, par1 = s.RetrievePmgLevel()[:2]
    s.ApplyPreconditioner(r)                                            # a second build from the same H
    off2, cols2, vals2 = s.RetrieveRestrictOp()
    out["r_bitwise_rebuild"] = bool(np.array_equal(off, off2) and np.array_equal(cols, cols2) and np.array_equal(vals, vals2))
    r_off, r_cols, r_vals, r_mag = rn.restricted_operator_blocks(f_off, f_cols, f_vals, sc_f, sc_c, par0, par1)
    out["r_pattern_equal"] = bool(np.array_equal(off, r_off) and np.array_equal(cols, r_cols))
    if out["r_pattern_equal"]:
        out["r_worst_excess"] = float((np.abs(vals - r_vals) - 2.0 ** -23 * r_mag).max())
        out["r_worst_rel"] = float((np.abs(vals - r_vals) / np.maximum(r_mag, 1e-300)).max())
        out["r_rows"] = [int(np.diff(off).min()), int(np.diff(off).max())]
    out["hook_lambda"] = list(s.GetLambdaMax())


def solves(s, out):
    n = 3 * s.n_coef
    rng = np.random.default_rng(3)
    out["solves"] = []
    for k in range(3):
        b = rng.normal(size=n)
        x, iters, rel = s.LinearSolve(b)
        lam = s.GetLambdaMax()
        true_res = float(np.linalg.norm(b - s.ApplyHessian(x)) / np.linalg.norm(b))
        out["solves"].append(dict(iters=int(iters), rel=float(rel), true_res=true_res, mode=s.GetSpmvMode(), lam=list(lam)))


def main(what, name):
    X, conn = gn.mesh(name)
    d, s, fixed, _, _ = pw.build_t10_mesh(X, conn)
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(1e-8, 0.0, 1e-8, 1e14, 2, 4, 1e-3))
    s.SetLinSolveOpts(tl.LinSolveOpts(REL_TOL, 20000, 10))
    s.EvalGradient()
    s.AssembleHessian()
    out = dict(mesh=name, what=what, assembly=s.GetAssemblyMode(), N=int(X.shape[0]), E=int(conn.shape[0]))
    if what == "full":
        galerkin_checks(s, out)
        restrict_op_checks(s, out)
    solves(s, out)
    out["precond"] = s.GetPreconditioner()
    out["cycle"] = s.GetPmgCycleInfo()
    print(json.dumps(out), flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
