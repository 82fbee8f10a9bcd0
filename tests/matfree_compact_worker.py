"""Scenarios of tests/test_gpu_matfree_compact.py.  TLFEA_SPMV_MATFREE and TLFEA_MATFREE_COMPACT are read once per
process, so each combination runs as `python -m tests.matfree_compact_worker <mesh> <npz out>` in a fresh child: y = H p
of the matrix-free pair for the test vectors, twice, the CSR product of the same H, two traced CG iterations for the raw
p.q slots, then one linear solve (with the CSR product or the pair, as TLFEA_SPMV_MATFREE says)."""
import sys

import numpy as np

from tests import matfree_worker as w
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_gpu

tl = w.tl


def mesh(name):
    """(X, conn): "small" 36 elements, under one wavefront; "box" 270 = 4 x 64 + 14 elements, 49 pinned nodes; "permuted"
    res4 (936 = 14 x 64 + 40 elements) in a seeded random element order: nodes with up to 15 compact rows"""
    if name == "small":
        return load_mesh("beam_3x2x1")
    if name == "box":
        return w.box_mesh()
    X, conn = load_mesh("res4")
    return X, np.ascontiguousarray(conn[np.random.default_rng(11).permutation(conn.shape[0])])


def vectors(X, conn, fixed):
    n = 3 * X.shape[0]
    vecs = [np.random.default_rng(5).normal(size=n)]
    for dof in (3 * int(fixed[0]) + 1, 3 * int(conn[0, 0]), 3 * int(conn[-1, 4]) + 2):   # pinned, corner, mid-edge of the last lane
        u = np.zeros(n)
        u[dof] = 1.0
        vecs.append(u)
    return np.stack(vecs)


def assembled(name):
    X, conn = mesh(name)
    fx = fixed_x0(X)
    d = make_gpu(X, conn, MATERIALS["svk"], fx, w.tip_load(X))
    s = w.make_solver(d)
    w.two_newton_iterations(s)      # F differs from I
    s.EvalGradient()
    s.AssembleHessian()
    assert s.GetAssemblyMode() == 3
    return X, conn, fx, d, s


def main(name, npz_out):
    X, conn, fx, d, s = assembled(name)
    P = vectors(X, conn, fx)
    y_csr = np.stack([s.ApplyHessian(p) for p in P])
    y = np.stack([s.ApplyHessianMatfree(p) for p in P])
    y_again = np.stack([s.ApplyHessianMatfree(p) for p in P])
    form, rows, ratio = s.GetMatfreeRows()
    out = dict(y=y, y_again=y_again, y_csr=y_csr, form=form, rows=rows, ratio=ratio, E=conn.shape[0], N=X.shape[0],
               n_fixed=len(fx))
    b = np.random.default_rng(3).normal(size=3 * X.shape[0])
    tr = s.CGTrace(b, 2)
    out.update(slots=tr["slots"], trace_matfree=tr["form"]["matfree"])
    x, iters, rel = s.LinearSolve(b)
    out.update(x=x, iters=iters, rel=rel, mode=s.GetSpmvMode(),
               true_res=float(np.linalg.norm(b - s.ApplyHessian(x)) / np.linalg.norm(b)))
    np.savez(npz_out, **out)
    del s
    d.Destroy()
    print(f"RESULT {name}: form {form}, {rows} rows, ratio {ratio:.3f}, solve mode {out['mode']}, {iters} iterations")


if __name__ == "__main__":
    main(*sys.argv[1:3])
