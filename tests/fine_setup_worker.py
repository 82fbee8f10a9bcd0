"""Worker of tests/test_gpu_fine_setup.py.  The library reads its TLFEA_* switches once per process, so every scenario runs as
`python -m tests.fine_setup_worker '<json config>' <out.npz>` in a fresh child (the caller sets the environment).  Prints
one JSON line last.

config: mesh (tests/galerkin_np.py: beam_3x2x1, box, permuted), explicit (true: cheb_bits = 16 from the first solve on),
hooks (false: the read-back of the fine copy and TimeKernels are left out; everything that solves stays); or what = "rop":
R of two set-ups and two solves, for the comparison of the two builds of R from H.

One script for every child, so that two children differ in nothing but what the test is about (the lambda_max estimate is
warm-started from solve to solve: equal histories give equal bits):

    phase 1 (automatic options, or explicit)   solve, solve, [read the fine copy back], solve, CGTrace, [TimeKernels], solve
    phase 2 (cheb_bits = 16 set explicitly)    solve, solve

After every operation the record holds the fine copy's state (bits allocated, current, conversions so far)."""
import json
import sys

import numpy as np

from tests import galerkin_np as gn
from tests import precond_worker as pw
from tests.helpers import tl

REL_TOL = 1e-12


def rop(cfg, out_path):
    """what = "rop": R as two set-ups of one H store it, then two solves (the caller sets TLFEA_ROP_BUILD / _STREAM_MAX)"""
    X, conn = gn.mesh(cfg["mesh"])
    d, s, fixed, _, _ = pw.build_t10_mesh(X, conn)
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(1e-8, 0.0, 1e-8, 1e14, 2, 4, 1e-3))
    s.SetLinSolveOpts(tl.LinSolveOpts(REL_TOL, 20000, 1))
    s.EvalGradient()
    s.AssembleHessian()
    n = 3 * s.n_coef
    r = np.random.default_rng(11).normal(size=n)
    s.ApplyPreconditioner(r)
    out = dict(mesh=cfg["mesh"], info=s.GetRestrictOpInfo(), smoother=s.GetFineSmoother())
    off, cols, vals = s.RetrieveRestrictOp()
    s.ApplyPreconditioner(r)                                            # a second build from the same H
    off2, cols2, vals2 = s.RetrieveRestrictOp()
    out["bitwise_rebuild"] = bool(np.array_equal(off, off2) and np.array_equal(cols, cols2) and np.array_equal(vals, vals2))
    out["rows"] = [int(np.diff(off).min()), int(np.diff(off).max())]
    b = np.random.default_rng(3).normal(size=n)
    data, out["solves"] = dict(off=off, cols=cols, vals=vals), []
    for k in range(2):
        x, its, rel = s.LinearSolve(b)
        true_res = float(np.linalg.norm(b - s.ApplyHessian(x)) / np.linalg.norm(b))
        out["solves"].append(dict(its=int(its), rel=float(rel), true_res=true_res, smoother=s.GetFineSmoother()))
        data["x%d" % k] = x
    out["state"] = list(s.GetFineCopyState())
    np.savez(out_path, **data)
    print(json.dumps(out), flush=True)
    del s
    d.Destroy()


def main(cfg, out_path):
    if cfg.get("what") == "rop":
        return rop(cfg, out_path)
    X, conn = gn.mesh(cfg["mesh"])
    d, s, fixed, _, _ = pw.build_t10_mesh(X, conn)
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(1e-8, 0.0, 1e-8, 1e14, 2, 4, 1e-3))
    auto, explicit = tl.LinSolveOpts(REL_TOL, 20000, 1), tl.LinSolveOpts(REL_TOL, 20000, 1, 0, 0.0, 16, 0)
    s.SetLinSolveOpts(explicit if cfg.get("explicit") else auto)
    s.EvalGradient()
    s.AssembleHessian()
    n = 3 * s.n_coef
    b = np.random.default_rng(3).normal(size=n)
    hooks = cfg.get("hooks", True)
    ops, data = [], {}

    def note(op, **kw):
        ops.append(dict(op=op, state=list(s.GetFineCopyState()), smoother=s.GetFineSmoother(), **kw))

    def solve(tag):
        x, its, rel = s.LinearSolve(b)
        true_res = float(np.linalg.norm(b - s.ApplyHessian(x)) / np.linalg.norm(b))
        data["x_" + tag] = x
        note("solve", tag=tag, its=int(its), rel=float(rel), true_res=true_res, finite=bool(np.all(np.isfinite(x))))

    solve("a0")
    solve("a1")
    if hooks:
        f_off, f_cols, f_vals, sc_f, sc_c = s.RetrieveFineCopy()
        data.update(f_off=f_off, f_cols=f_cols, f_vals=f_vals, sc_f=sc_f, sc_c=sc_c)
        note("retrieve")
    solve("a2")
    tr = s.CGTrace(b, 2)
    note("trace", graphs=tr["form"]["graphs"], matfree=tr["form"]["matfree"])
    if hooks:
        t = s.TimeKernels(reps=2)
        note("time", cheb_step=float(t["cheb_step"]), cheb_step_cycle=float(t["cheb_step_cycle"]))
    solve("a3")
    s.SetLinSolveOpts(explicit)
    solve("e0")
    solve("e1")
    np.savez(out_path, **data)
    print(json.dumps(dict(mesh=cfg["mesh"], N=int(X.shape[0]), ops=ops, precond=s.GetPreconditioner(), cycle=s.GetPmgCycleInfo())),
          flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    main(json.loads(sys.argv[1]), sys.argv[2])
