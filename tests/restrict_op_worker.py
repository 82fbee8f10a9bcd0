"""Worker of tests/test_gpu_restrict_op.py (the library reads its TLFEA_* switches once per process; the caller sets the
environment).

    python tests/restrict_op_worker.py build    '<json config>' <out.npz>   R against its definition, two builds
    python tests/restrict_op_worker.py operator '<json config>' <out.npz>   tests/precond_worker.py + which path ran
    python tests/restrict_op_worker.py newton   '<json config>' <out.npz>   one Newton step: iteration count, velocities

Every mode prints one JSON line last."""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import precond_worker as pw  # noqa: E402
from tests import restricted_op_np as rn  # noqa: E402
from tests.helpers import tl  # noqa: E402


def build(cfg, out_path):
    d, s, fixed, trans, rot = pw.build_t10(cfg["problem"])
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-4, 1e-4, 1e14, 5, 10, 1e-3))
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 20000, 1, *cfg["opts"]))
    s.AssembleHessian()
    n = 3 * s.n_coef
    r = np.random.default_rng(11).normal(size=n)
    s.ApplyPreconditioner(r)
    info = s.GetRestrictOpInfo()
    out = dict(name=cfg["name"], info=info)
    assert info["active"] == 1, info
    off, cols, vals = s.RetrieveRestrictOp()
    f_off, f_cols, f_vals, sc_f, sc_c = s.RetrieveFineCopy()
    par0, par1 = s.RetrievePmgLevel()[:2]
    s.ApplyPreconditioner(r)                                            # a second build from the same H
    off2, cols2, vals2 = s.RetrieveRestrictOp()
    out["bitwise_rebuild"] = bool(np.array_equal(off, off2) and np.array_equal(cols, cols2) and np.array_equal(vals, vals2))
    # the stored copy holds what its type can hold, R what float32 can
    store = info["fine_bits"]
    out["copy_is_stored_type"] = bool(np.array_equal(f_vals, f_vals.astype(np.float16 if store == 16 else np.float32).astype(np.float64)))
    out["r_is_float32"] = bool(np.array_equal(vals, vals.astype(np.float32).astype(np.float64)))
    r_off, r_cols, r_vals, r_mag = rn.restricted_operator_blocks(f_off, f_cols, f_vals, sc_f, sc_c, par0, par1)
    out["pattern_equal"] = bool(np.array_equal(off, r_off) and np.array_equal(cols, r_cols))
    if out["pattern_equal"]:
        excess = np.abs(vals - r_vals) - 2.0 ** -23 * r_mag
        out["worst_excess"] = float(excess.max())
        out["worst_rel"] = float((np.abs(vals - r_vals) / np.maximum(r_mag, 1e-300)).max())
        out["rows_max"], out["rows_min"] = int(np.diff(off).max()), int(np.diff(off).min())
        out["fine_rows_max"], out["fine_rows_min"] = int(np.diff(f_off).max()), int(np.diff(f_off).min())
    print(json.dumps(out), flush=True)
    del s
    d.Destroy()


def operator(cfg, out_path):
    seen = {}
    solve = tl.SyncedNewtonSolver.LinearSolve

    def solve_and_look(self, b):                                        # which path did the solve's set-up choose?
        res = solve(self, b)
        seen.update(self.GetRestrictOpInfo())
        ro, ci, val = self.RetrieveHessianCSRToCPU()
        H = sp.csr_matrix((val, ci, ro), shape=(len(b), len(b)))
        seen["true_rel"] = float(np.linalg.norm(b - H @ res[0]) / np.linalg.norm(b))
        return res
    tl.SyncedNewtonSolver.LinearSolve = solve_and_look
    pw.main(cfg, out_path)                                              # prints its JSON line
    print(json.dumps(seen), flush=True)


def newton(cfg, out_path):
    d, s, fixed, trans, rot = pw.build_t10(cfg["problem"])
    s.SetParameters(tl.SyncedNewtonParams(1e-6, 0.0, 1e-6, 1e14, 1, 1, 1e-3))
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 20000, 1, 0, 0.0, 0, 0))
    s.Solve()
    st = s.GetStats()
    info = s.GetRestrictOpInfo()
    np.savez(out_path, v=s.RetrieveVelocityToCPU())
    print(json.dumps(dict(name=cfg["name"], pcg_iters=st["pcg_iters"], newton=st["newton"], active=info["active"],
                          precond=s.GetPreconditioner())), flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    {"build": build, "operator": operator, "newton": newton}[sys.argv[1]](json.loads(sys.argv[2]), sys.argv[3])
