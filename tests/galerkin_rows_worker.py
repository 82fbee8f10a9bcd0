"""Worker of tests/test_gpu_galerkin_rows.py.  The library reads its TLFEA_* switches once per process, so every
configuration runs as `python -m tests.galerkin_rows_worker '<json config>' <out.npz>` in a fresh child (the caller sets the
environment).  Prints one JSON line last.

config: mesh (tests/galerkin_np.py: beam_3x2x1, box, permuted).  One script for every child, so that two children differ in
nothing but the switches the test is about:

    set-up (ApplyPreconditioner)   Hc as built + the kernel that built it, R if the set-up built one
    set-up again, same H           Hc as built (bit for bit the first?), the vertex level's scaling sc_c
    stand-alone read-back          Hc summed again by RetrievePmgLevel, with the parent map and the coarse pattern
    NumPy                          P^T H P of the H on the device: relative error and off-diagonal asymmetry of the as-built Hc
    two solves from one right-hand side"""
import json
import sys

import numpy as np
import scipy.sparse as sp

from tests import galerkin_np as gn
from tests import galerkin_rows_np as grn
from tests import precond_worker as pw
from tests.helpers import tl

REL_TOL = 1e-12


def main(cfg, out_path):
    X, conn = gn.mesh(cfg["mesh"])
    d, s, fixed, _, _ = pw.build_t10_mesh(X, conn)
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(1e-8, 0.0, 1e-8, 1e14, 2, 4, 1e-3))
    s.SetLinSolveOpts(tl.LinSolveOpts(REL_TOL, 20000, 1))
    s.EvalGradient()
    s.AssembleHessian()
    n = 3 * s.n_coef
    r = np.random.default_rng(11).normal(size=n)
    out, data = dict(mesh=cfg["mesh"]), {}
    s.ApplyPreconditioner(r)
    hc, out["form"] = s.RetrievePmgLevelBuilt()
    out["smoother"], out["info"] = s.GetFineSmoother(), s.GetRestrictOpInfo()
    out["precond"], out["cycle"] = s.GetPreconditioner(), s.GetPmgCycleInfo()
    if out["info"]["active"]:
        data["r_off"], data["r_cols"], data["r_vals"] = s.RetrieveRestrictOp()
    s.ApplyPreconditioner(r)                                            # a second set-up from the same H
    hc2, form2 = s.RetrievePmgLevelBuilt()
    out["bitwise_rebuild"] = bool(form2 == out["form"] and np.array_equal(hc, hc2))
    data["sc_c"] = s.RetrieveFineCopy()[4]                              # what the set-up scaled the vertex level (and R) with
    par0, par1, c_off, c_cols, hc_alone = s.RetrievePmgLevel()          # sums Hc again, on its own
    data.update(hc=hc, hc_alone=hc_alone, c_off=c_off, c_cols=c_cols)
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    H = sp.csr_matrix((val, ci, ro), shape=(n, n))
    nc = len(c_off) - 1
    P = gn.prolongation(par0, par1, nc)
    ref = (P.T @ H @ P).tocsr()
    out["hc_relerr"] = float(abs(gn.dof_csr(c_off, c_cols, hc) - ref).max() / abs(ref).max())
    out["hc_asym_offdiag"] = grn.off_diagonal_asymmetry(c_off, c_cols, hc)
    out["hc_max"] = float(abs(ref).max())
    b = np.random.default_rng(3).normal(size=n)
    out["solves"] = []
    for k in range(2):
        x, its, rel = s.LinearSolve(b)
        true_res = float(np.linalg.norm(b - s.ApplyHessian(x)) / np.linalg.norm(b))
        out["solves"].append(dict(its=int(its), rel=float(rel), true_res=true_res, smoother=s.GetFineSmoother(),
                                  finite=bool(np.all(np.isfinite(x)))))
        data["x%d" % k] = x
    np.savez(out_path, **data)
    print(json.dumps(out), flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    main(json.loads(sys.argv[1]), sys.argv[2])
