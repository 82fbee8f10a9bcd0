"""Scenarios of tests/test_gpu_matfree_records.py.  TLFEA_MATFREE_POINTS, TLFEA_SPMV_MATFREE, TLFEA_MATFREE_COMPACT and
TLFEA_PMG_FINE_MATFREE are read once per process, so each combination runs as `python -m tests.matfree_records_worker
<mesh> <npz out>` in a fresh child on a mesh of tests/matfree_compact_worker.py: the product of the matrix-free pair for
the test vectors (twice) and the CSR product of the same H, the element-major and the packed records, one linear solve
(whose preconditioner set-up packs the float records where it takes the fine smoother from them), then a further Newton
iteration and assembly: the product of the new generation, and one smoother pass against the records of the old one."""
import sys

import numpy as np

from tests import matfree_compact_worker as mcw
from tests import matfree_worker as w


def records(s, out, tag, single):
    pts, gp = s.GetMatfreeRecords(2, single)
    pts2, Fp = s.GetMatfreeRecords(3, single)
    assert pts == pts2
    out.update({"gp" + tag: gp, "Fp" + tag: Fp, "points" + tag: pts})


def main(name, npz_out):
    X, conn, fx, d, s = mcw.assembled(name)
    n = 3 * X.shape[0]
    P = mcw.vectors(X, conn, fx)
    y_csr = np.stack([s.ApplyHessian(p) for p in P])
    y = np.stack([s.ApplyHessianMatfree(p) for p in P])
    y_again = np.stack([s.ApplyHessianMatfree(p) for p in P])
    out = dict(y=y, y_again=y_again, y_csr=y_csr, form=s.GetMatfreeRows()[0], E=conn.shape[0], N=X.shape[0])
    out["gvec"], out["Fq"] = s.GetMatfreeRecords(0)[1], s.GetMatfreeRecords(1)[1]
    records(s, out, "64", False)

    b = np.random.default_rng(3).normal(size=n)
    x, iters, rel = s.LinearSolve(b)
    out.update(x=x, iters=iters, rel=rel, mode=s.GetSpmvMode(), fine=s.GetFineSmoother(),
               true_res=float(np.linalg.norm(b - s.ApplyHessian(x)) / np.linalg.norm(b)))
    if out["fine"] == 1:                         # the set-up of that solve packed the float records of this H
        records(s, out, "32", True)

    # a further Newton iteration and assembly: another generation of records
    s.NewtonIteration()
    s.EvalGradient()
    s.AssembleHessian()
    out["y2_csr"], out["y2"] = s.ApplyHessian(P[0]), s.ApplyHessianMatfree(P[0])
    out["Fq2"] = s.GetMatfreeRecords(1)[1]
    pts, out["Fp2"] = s.GetMatfreeRecords(3)
    stale = ""
    if out["fine"] == 1:                         # the float records are still those of the solve's H
        z = np.zeros(n, dtype=np.float32)
        try:
            s.FineSmootherPass(z, z, z, np.zeros(n), [1.0, 1.0])
            stale = "accepted"
        except w.TlfeaError as e:
            stale = str(e)
    out["stale"] = stale
    np.savez(npz_out, **out)
    del s
    d.Destroy()
    print(f"RESULT {name}: {out['points64']} points, form {out['form']}, solve mode {out['mode']}, fine smoother {out['fine']}, "
          f"{iters} iterations")


if __name__ == "__main__":
    main(*sys.argv[1:3])
