"""The flag of the 12 x 12 node-block factorisation (blk12_factor_kernel, csrc/solver_kernels.hip) that the polynomial
preconditioner of the ANCF kinds sets up with: a node block of H that is not positive definite refuses the solve, by name --
and only that solve.  The flag reports one factorisation: once H is SPD again (a rolled-back trial step), the same solver
object solves again, through both readers of the flag (the CG's set-up in csrc/cg_api.hip, precond_setup_whole in
csrc/precond_api.hip behind ApplyPreconditioner).

Three shells (tests/test_gpu_ancf.py::shell_problem), SVK without damping, h = 1e-3, default solve options.  All
coefficients scaled by 0.7 compress the shells: the oracle's H of that state has a 12 x 12 node block with smallest
eigenvalue -1.9e4 (asserted below, on the CPU); at the reference state the smallest is +1.0e3 and H has smallest eigenvalue
2.9e2.  Bounds of the good solve (tests/test_gpu_precond_operator.py): relative residual <= 1e-12 -- the true one, b - H x
with the downloaded H in numpy -- and x against numpy's solve of the oracle's H to 1e-8 of its largest entry.  Measured
on the MI355X: 15 iterations, true residual 1.2e-14 to 1.8e-14, x to 9e-15; the operator after a refused set-up is that of
a solver that never saw the bad H, bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

import tests.test_gpu_ancf as A
from tests.helpers import relerr, tl
from tests.test_gpu_parity import TOL_ELEM

pytestmark = pytest.mark.gpu
H_STEP, RHO = 1e-3, 1e14
REFUSAL = "12 x 12 node block of H is not positive definite"


def oracle_h(o, scale):
    o.x, o.y, o.z = scale * o.xt, scale * o.yt, scale * o.zt
    ro, ci, val = o.assemble_hessian(H_STEP, RHO)
    n = len(ro) - 1
    return sp.csr_matrix((val, ci, ro), shape=(n, n))


def min_node_block_eigenvalue(H):
    D = H.toarray()
    return min(np.linalg.eigvalsh(D[k:k + 12, k:k + 12]).min() for k in range(0, D.shape[0], 12))


def new_solver(d):
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 0.0, 1e-6, RHO, 5, 10, H_STEP))
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-13, 50000, 10))      # the preconditioner's options all at their defaults
    return s


def set_state(d, o, scale):
    d.UpdatePositions(scale * o.xt, scale * o.yt, scale * o.zt)


def test_a_node_block_that_is_not_spd_refuses_that_solve_only():
    o, d = A.make_pair(A.PROBLEMS["shell3443"](), A.SVK)
    assert o.E == 3
    H_bad, H_good = oracle_h(o, 0.7), oracle_h(o, 1.0)
    eig_bad, eig_good, eig_h = min_node_block_eigenvalue(H_bad), min_node_block_eigenvalue(H_good), np.linalg.eigvalsh(H_good.toarray()).min()
    print("smallest eigenvalue of the 12 x 12 node blocks: %.3e at scale 0.7, %.3e at the reference; of H there: %.3e" % (eig_bad, eig_good, eig_h))
    assert eig_bad < -1e4 and eig_good > 1e2 and eig_h > 1e2      # the CPU precondition of both outcomes
    n = H_good.shape[0]
    rng = np.random.default_rng(3)
    b, r = rng.normal(size=n), rng.normal(size=n)
    x_np = np.linalg.solve(H_good.toarray(), b)

    # the operator of the reference state on a solver that never saw the bad H (ApplyPreconditioner sets up from cold
    # estimates started at r and leaves the warm state alone: a function of H and r)
    fresh = new_solver(d)
    fresh.AssembleHessian()
    z_fresh = fresh.ApplyPreconditioner(r)
    del fresh

    s = new_solver(d)
    assert s.GetPolynomialInfo()["block"] == 12 and s.GetPreconditioner() == 1       # the node-block scaling is active

    def bad_state(call):
        set_state(d, o, 0.7)
        s.AssembleHessian()
        ro, ci, val = s.RetrieveHessianCSRToCPU()
        assert relerr(val, H_bad.data) < TOL_ELEM                  # the H the precondition was computed for
        with pytest.raises(tl.TlfeaError, match=REFUSAL):
            call()

    def good_solve(step):
        set_state(d, o, 1.0)
        s.AssembleHessian()
        ro, ci, val = s.RetrieveHessianCSRToCPU()
        assert np.array_equal(ro, H_good.indptr) and np.array_equal(ci, H_good.indices) and relerr(val, H_good.data) < TOL_ELEM
        x, its, rel = s.LinearSolve(b)
        true_rel = np.linalg.norm(b - sp.csr_matrix((val, ci, ro), shape=(n, n)) @ x) / np.linalg.norm(b)
        x_err = np.abs(x - x_np).max() / np.abs(x_np).max()
        print("step %s: %d iterations, reported residual %.2e, true residual %.2e, x against numpy %.2e" % (step, its, rel, true_rel, x_err))
        assert s.GetPreconditionerState()["block"] == 12
        assert rel <= 1e-12 and true_rel <= 1e-12 and x_err <= 1e-8

    # steps 1 and 2: the reader in the CG's set-up
    bad_state(lambda: s.LinearSolve(b))
    good_solve("2")
    # step 3: the reader behind the operator hook (precond_setup_whole), then the CG once more
    bad_state(lambda: s.ApplyPreconditioner(r))
    set_state(d, o, 1.0)
    s.AssembleHessian()
    z = s.ApplyPreconditioner(r)
    print("step 3: r.z / (|r| |z|) %.3e, max |z - z_fresh| %.3e" % (float(r @ z) / (np.linalg.norm(r) * np.linalg.norm(z)), np.abs(z - z_fresh).max()))
    assert np.all(np.isfinite(z)) and r @ z > 0.0
    assert np.array_equal(z, z_fresh)                              # the operator of a solver that never saw the bad H
    good_solve("3")
    bad_state(lambda: s.ApplyPreconditioner(np.stack([r, b])))     # the block form of the hook reads it too
    good_solve("3, after the block hook")
    del s
    d.Destroy()
