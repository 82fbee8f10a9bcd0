"""CPU checks of the modal solve's NumPy statement (tests/modal_np.py) on the oracle's H and M, and that the
library exposes the modal entry points.

The reference is scipy.linalg.eigh of the reduced dense pencil.  The oracle's (= the reference code's) T10 mass matrix
comes from the 5-point Keast rule, whose centroid weight is negative: it is symmetric but NOT positive definite, so
eigh(K, M) -- which factorises its second argument -- raises on it.  The same pencil is therefore handed over as
eigh(M, A), A = K + sigma M (SPD): its eigenvalues are theta = 1 / (omega^2 + sigma), the physical modes the largest.

Iteration counts of the block-Jacobi model at tol 1e-8 (recorded from this file's run; the cap is the 500 the GPU tests use):
clamped beam_3x2x1, sigma (2 pi)^2: 77 (SVK), 96 (neo-Hookean); free cube, sigma 1e4: 41 -- at (2 pi)^2 block-Jacobi alone does not get the
free cube's six rigid-body modes next to omega_7^2 = 1.3e6 within 500 iterations, hence the larger shift here; random
SPD pencil of 60 DOF: 17.
"""
import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from tests import modal_np as mn
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_oracle, tl

CAP = 500
TOL = 1e-8


def oracle_pencil(tag, mat, clamp, sigma):
    X, conn = load_mesh(tag)
    fixed = fixed_x0(X) if clamp else None
    o = make_oracle(X, conn, MATERIALS[mat], fixed)
    h = 1.0 / np.sqrt(sigma)
    ro, ci, val = o.assemble_hessian(h, 1e14)
    n = 3 * X.shape[0]
    A = sp.csr_matrix((val, ci, ro), shape=(n, n)) * (1.0 / h)
    Mn = sp.csr_matrix((o.m_val, o.m_col, o.m_off), shape=(n // 3, n // 3))
    M = sp.kron(Mn, sp.identity(3)).tocsr()
    free = np.ones(n, dtype=bool)
    if clamp:
        free[(3 * fixed[:, None] + np.arange(3)).reshape(-1)] = False
    return A, M, free


def dense_mu(A, M, free, k):
    """the k lowest positive mu of A phi = mu M phi on the free DOFs, and their M-normalised vectors"""
    Ad, Md = A.toarray()[np.ix_(free, free)], M.toarray()[np.ix_(free, free)]
    th, V = sl.eigh(Md, Ad)
    th, V = th[::-1][:k], V[:, ::-1][:, :k]
    return 1.0 / th, V / np.sqrt(th)[None, :]


def check(A, M, free, res, n_modes, sigma):
    mu, _ = dense_mu(A, M, free, n_modes)
    assert res["converged"] == n_modes and res["iterations"] <= CAP
    # residual <= tol mu |M phi| bounds the eigenvalue error by order tol mu; the error is quadratic in it
    assert np.all(np.abs(res["mu"] - mu) <= 2 * TOL * mu)
    Phi = res["modes"]
    assert not Phi[~free].any()
    assert np.allclose(Phi.T @ (M @ Phi), np.eye(n_modes), atol=1e-10)
    MP = (M @ Phi)[free]
    R = (A @ Phi)[free] - MP * res["mu"][None, :]
    assert np.all(np.linalg.norm(R, axis=0) <= 2 * TOL * res["mu"] * np.linalg.norm(MP, axis=0))


@pytest.mark.parametrize("mat", ["svk", "neo"])
def test_clamped_beam(mat):
    sigma = (2 * np.pi) ** 2
    A, M, free = oracle_pencil("beam_3x2x1", mat, True, sigma)
    res = mn.lobpcg(A, M, mn.block_jacobi(A, len(free) // 3), free, 6, tol=TOL, max_iter=CAP)
    print(mat, "iterations", res["iterations"], "omega2", res["mu"] - sigma)
    check(A, M, free, res, 6, sigma)


def test_free_cube_rigid_body_modes():
    sigma = 1e4
    A, M, free = oracle_pencil("cube", "svk", False, sigma)
    assert np.linalg.eigvalsh(M.toarray()).min() < 0.0   # the indefinite mass matrix the formulation has to live with
    res = mn.lobpcg(A, M, mn.block_jacobi(A, len(free) // 3), free, 10, tol=TOL, max_iter=CAP)
    print("iterations", res["iterations"], "omega2", res["mu"] - sigma)
    check(A, M, free, res, 10, sigma)
    w2 = res["mu"] - sigma
    assert np.all(np.abs(w2[:6]) <= 1e-8 * w2[6])


def test_random_spd_pencil():
    rng = np.random.default_rng(3)
    n = 60
    # a banded SPD A whose 3 x 3 diagonal blocks carry most of it (what block-Jacobi is a preconditioner for) with a
    # spectrum over three decades, and a dense SPD M
    d = np.geomspace(1.0, 1e3, n)
    E = np.triu(np.tril(rng.normal(size=(n, n)), 4), -4)
    A = np.diag(d) + 0.1 * np.sqrt(np.outer(d, d)) * (E + E.T) / 2
    B = rng.normal(size=(n, n))
    M = 0.2 * B @ B.T / n + np.eye(n)
    assert np.linalg.eigvalsh(A).min() > 0.0
    A, M = 0.5 * (A + A.T), 0.5 * (M + M.T)
    free = np.ones(n, dtype=bool)
    res = mn.lobpcg(A, M, mn.block_jacobi(A, n // 3), free, 5, tol=TOL, max_iter=CAP)
    print("iterations", res["iterations"])
    check(sp.csr_matrix(A), sp.csr_matrix(M), free, res, 5, 0.0)


def test_start_block_and_dense_helpers():
    a, b = mn.hash_block(30, 4, 7), mn.hash_block(30, 4, 7)
    assert np.array_equal(a, b) and not np.array_equal(a, mn.hash_block(30, 4, 8))
    assert a.min() >= -1.0 and a.max() < 1.0 and abs(a.mean()) < 0.3
    rng = np.random.default_rng(0)
    B = rng.normal(size=(12, 8))
    B[:, 1] = 2.0 * B[:, 0]                              # a dependent column: the Cholesky path must hand over to SVQB
    GA, GM = B.T @ B, np.diag(np.arange(1.0, 9.0))
    assert mn.cholesky_lower(GA / np.sqrt(np.outer(np.diag(GA), np.diag(GA))), mn.CHOL_PIVOT_MIN) is None
    th, C = mn.rayleigh_ritz(GA, GM, 3)
    assert np.all(np.diff(th) <= 0) and np.allclose(C.T @ GA @ C, np.eye(3), atol=1e-9)


def test_library_has_the_modal_entry_points():
    lib = tl.load_library()
    for name in ("tlfea_newton_modal_solve", "tlfea_newton_modal_apply_block", "tlfea_newton_modal_gram"):
        assert name in tl.exported_symbols() and hasattr(lib, name)
    assert hasattr(tl.SyncedNewtonSolver, "ModalAnalysis")
