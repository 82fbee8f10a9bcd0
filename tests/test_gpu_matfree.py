"""Matrix-free Hessian product of the CG iteration against the CSR product of the assembled H.

The product must be the SAME operator to rounding: 1e-12 relative to max |y| (the project's bound for H against the
oracle), bit-identical from call to call, and a linear solve that uses it reaches the same tolerance and the same
solution.  Where it is not eligible the CSR kernel runs (mode 0) and the test entry point returns an error."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import matfree_worker as w

tl = importlib.import_module("total-lagrangian-fea_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12

# TRUE residual ||b - H x|| / ||b|| (host, from ApplyHessian) that the CSR solve leaves on the cases of
# test_forced_on_solve_matches_the_csr_solve (rel_tol 1e-12, measured once on MI355X with the CSR kernel, whose code path
# is the parent commit's; the matrix-free solves left 5.330130e-13 and 4.448500e-13 in 16 and 19 iterations, as many as
# the CSR solves).  The recurrence residual and the true one drift apart by rounding only, hence the factor 2 below.
PARENT_TRUE_RES = {"box": 5.330108e-13, "res4": 4.448492e-13}


def child(args, env_value):
    env = dict(os.environ, TLFEA_SPMV_MATFREE=env_value)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "tests.matfree_worker"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("mesh", ["box", "res4"])
def test_product_equals_the_csr_product(mesh):
    X, conn, fixed, d = w.make_case(mesh)
    s = w.make_solver(d)
    w.two_newton_iterations(s)      # F differs from I
    s.EvalGradient()
    s.AssembleHessian()
    assert s.GetAssemblyMode() == 3
    n = 3 * X.shape[0]
    vecs = [("random", np.random.default_rng(5).normal(size=n))]
    for name, dof in (("clamped DOF", 3 * int(fixed[0]) + 1), ("corner node", 3 * int(conn[0, 0])),
                      ("mid-edge node", 3 * int(conn[0, 4]) + 2)):
        u = np.zeros(n)
        u[dof] = 1.0
        vecs.append((name, u))
    for name, p in vecs:
        y_ref = s.ApplyHessian(p)
        y = s.ApplyHessianMatfree(p)
        err = float(np.max(np.abs(y - y_ref)) / np.max(np.abs(y_ref)))
        print(f"{mesh} {name}: max |y_mf - y_csr| / max |y_csr| = {err:.3e}")
        assert err < TOL, (name, err)
        assert np.array_equal(s.ApplyHessianMatfree(p), y), name      # bitwise reproducible
    del s
    d.Destroy()


def test_records_of_another_state_are_refused():
    """a residual evaluation after the assembly rewrites the F records: the product must not pair them with the old H"""
    X, conn, fixed, d = w.make_case("res2")
    s = w.make_solver(d)
    w.two_newton_iterations(s)
    s.EvalGradient()
    s.AssembleHessian()
    p = np.ones(3 * X.shape[0])
    s.ApplyHessianMatfree(p)
    s.EvalGradient()
    with pytest.raises(w.TlfeaError, match="not eligible"):
        s.ApplyHessianMatfree(p)
    s.AssembleHessian()
    y = s.ApplyHessianMatfree(p)
    y_ref = s.ApplyHessian(p)
    assert float(np.max(np.abs(y - y_ref)) / np.max(np.abs(y_ref))) < TOL
    del s
    d.Destroy()


@pytest.mark.parametrize("mesh", ["box", "res4"])
def test_forced_on_solve_matches_the_csr_solve(mesh, tmp_path):
    ref = w.solve_case(mesh)        # this process: small mesh, default switch -> the CSR kernel
    assert ref["mode"] == 0 and ref["rel"] <= w.REL_TOL
    npz = str(tmp_path / "ref.npz")
    np.savez(npz, **ref)
    out = child(["solve", mesh, npz], "1")
    m = re.search(r"RESULT .* x_err=(\S+) true_res=(\S+) true_res_csr=(\S+)", out)
    assert m, out
    x_err, true_res, true_res_csr = (float(v) for v in m.groups())
    print(out.strip().splitlines()[-1])
    assert x_err <= 1e-10, x_err    # the displacement parity bound of the suite
    assert true_res <= 2.0 * PARENT_TRUE_RES[mesh], (true_res, PARENT_TRUE_RES[mesh])


@pytest.mark.parametrize("which", ["mooney_rivlin", "obstacle", "linear_constraint", "curved"])
def test_ineligible_cases_keep_the_csr_kernel(which):
    out = child(["ineligible", which], "1")     # forced on: still not eligible
    assert f"RESULT ineligible {which}" in out, out
