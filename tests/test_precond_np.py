"""tests/precond_np.py (the fp64 restatement of the CG preconditioner the GPU tests compare the device with) checked
against mathematics, on H from the oracle: the T10 beam_3x2x1 mesh and the 3-element ANCF shell strip."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import orc
from tests import precond_np as pn
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_oracle

EDGES = [(0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3)]


@pytest.fixture(scope="module")
def t10():
    """H at a perturbed state with x = 0 pinned (penalty 1e14), the vertex hierarchy and a hand-made third level"""
    X, conn = load_mesh("beam_3x2x1")
    fixed = fixed_x0(X)
    o = make_oracle(X, conn, MATERIALS["svk"], fixed)
    x = X + np.random.default_rng(7).normal(0.0, 1e-4, X.shape)
    x[fixed] = X[fixed]
    o.x, o.y, o.z = (np.ascontiguousarray(x[:, i]) for i in range(3))
    ro, ci, val = o.assemble_hessian(1e-3, 1e14)
    N = X.shape[0]
    H = sp.csr_matrix((val, ci, ro), shape=(3 * N, 3 * N))
    verts = np.unique(conn[:, :4])
    cid = -np.ones(N, dtype=np.int64)
    cid[verts] = np.arange(len(verts))
    par0, par1 = cid.copy(), cid.copy()
    for m, (a, b) in enumerate(EDGES):
        par0[conn[:, 4 + m]], par1[conn[:, 4 + m]] = cid[conn[:, a]], cid[conn[:, b]]
    P = pn.prolongation_p(par0, par1, len(verts))
    Hc = (P.T @ H @ P).tocsr()
    # third level: vertices binned along x into 4 aggregates; the last one keeps translations only (rotations off)
    Xv = X[verts]
    agg = np.minimum((Xv[:, 0] / (Xv[:, 0].max() + 1e-9) * 4).astype(np.int64), 3)
    rvec = Xv - np.stack([Xv[agg == A].mean(axis=0) for A in range(4)])[agg]
    active = np.array([1, 1, 1, 0])
    rvec[agg == 3] = 0.0
    P2 = pn.prolongation_rbm(agg, rvec, 4)
    H3 = pn.level3_matrix(Hc, P2, active)
    return dict(H=H, P=P, Hc=Hc, P2=P2, H3=H3, n=3 * N)


@pytest.fixture(scope="module")
def shell():
    from tests.test_gpu_ancf import SVK, shell_problem
    kind, x, y, z, conn, (L, W, Hh), fixed, f_ext = shell_problem()
    mat = orc.svk(SVK["E"], SVK["nu"], rho0=SVK["rho0"], eta=0.0, lamd=0.0)
    o = orc.AncfOracle(kind, x, y, z, conn, L, W, Hh, mat, fixed, f_ext)
    o.calc_dsdu_pre()
    o.calc_mass()
    rng = np.random.default_rng(5)
    o.x, o.y, o.z = (a + rng.normal(0, 1e-3, a.shape) for a in (o.xt, o.yt, o.zt))
    ro, ci, val = o.assemble_hessian(1e-3, 1e14)
    n = 3 * len(x)
    return dict(H=sp.csr_matrix((val, ci, ro), shape=(n, n)), n=n)


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def cheb_q(lam, lam_hi, kappa, terms):
    """q(lam) = (1 - T_k((theta - lam) / delta) / T_k(theta / delta)) / lam with T_k from its three-term recurrence:
    the polynomial `terms` terms of the Chebyshev iteration from z = 0 apply to the right-hand side"""
    b, a = lam_hi, lam_hi / kappa
    theta, delta = 0.5 * (b + a), 0.5 * (b - a)

    def T(x):
        t0, t1 = np.ones_like(x), x
        for _ in range(terms - 1):
            t0, t1 = t1, 2.0 * x * t1 - t0
        return t1
    return (1.0 - T((theta - lam) / delta) / T(np.array(theta / delta))) / lam


def inv_sqrt_blocks(D):
    w, V = np.linalg.eigh(D)
    return np.einsum("nij,nj,nkj->nik", V, 1.0 / np.sqrt(w), V)


@pytest.mark.parametrize("which", ["t10", "shell"])
@pytest.mark.parametrize("terms,kappa", [(12, 400.0), (24, 1600.0)])
def test_polynomial_is_q_of_the_scaled_matrix(which, terms, kappa, request):
    p = request.getfixturevalue(which)
    lvl = pn.Level(p["H"], 64)
    lam = 1.15 * pn.lam_max_dinv_h(lvl)
    coef = np.array(pn.chebyshev_pairs(lam, kappa, terms)).reshape(-1)
    M = pn.dense_of(pn.polynomial(lvl, coef, terms), p["n"])
    Dh = sp.block_diag(list(inv_sqrt_blocks(pn.diag_blocks(p["H"]))), format="csr").toarray()   # D^-1/2, block by block
    w, V = np.linalg.eigh(Dh @ p["H"].toarray() @ Dh)
    ref = Dh @ (V * cheb_q(w, lam, kappa, terms)) @ V.T @ Dh
    assert relmax(M, ref) < 1e-10


def t10_states(p, store):
    f, c, l3 = pn.Level(p["H"], store), pn.Level(p["Hc"], store), pn.Level(p["H3"], store)
    lf, lc, l33 = (1.15 * pn.lam_max_dinv_h(v) for v in (f, c, l3))
    two = pn.cycle_state(pn.chebyshev_pairs(lf, 24.0, 4), pn.chebyshev_pairs(lc, 216.0, 12))
    three = pn.cycle_state(pn.chebyshev_pairs(lf, 8.0, 2), pn.chebyshev_pairs(lc, 90.0, 6), pn.chebyshev_pairs(l33, 96.0, 8))
    return f, c, l3, two, three


@pytest.mark.parametrize("store", [16, 32, 64])
def test_every_operator_is_symmetric_positive_definite(t10, shell, store):
    f, c, l3, two, three = t10_states(t10, store)
    lam = 1.15 * pn.lam_max_dinv_h(f)
    coef = np.array(pn.chebyshev_pairs(lam, 1600.0, 24)).reshape(-1)
    ops = {"polynomial": (pn.polynomial(f, coef, 24), t10["n"]),
           "two_level": (pn.two_level_cycle(f, c, t10["P"], two), t10["n"]),
           "three_level": (pn.three_level_cycle(f, c, l3, t10["P"], t10["P2"], three), t10["n"])}
    fk, betas = pn.fourth_kind_pairs(lam, 4)
    four = pn.cycle_state(fk, pn.chebyshev_pairs(1.15 * pn.lam_max_dinv_h(c), 216.0, 12), betas=betas)
    ops["two_level_fourth_kind"] = (pn.two_level_cycle(f, c, t10["P"], four), t10["n"])
    nb0 = pn.node_block_form(shell["H"], None, 0, 64)
    lam_s = 1.15 * float(np.linalg.eigvalsh(nb0.Hhat.toarray()).max())
    coef_s = np.array(pn.chebyshev_pairs(lam_s, 200.0, 16)).reshape(-1)
    ops["node_block"] = (pn.node_block_form(shell["H"], coef_s, 16, store), shell["n"])
    for name, (op, n) in ops.items():
        M = pn.dense_of(op, n)
        assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max(), name
        assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0, name


def test_two_level_cycle_with_exact_coarse_solve_is_the_textbook_form(t10):
    """z1 = B r ; z2 = z1 + C (r - H z1) ; z = z2 + B (r - H z2) with B the smoother polynomial and C = P Hc^-1 P^T,
    multiplied out densely"""
    f, c, _, two, _ = t10_states(t10, 64)
    H, P, Hc = t10["H"].toarray(), t10["P"].toarray(), t10["Hc"].toarray()
    n = t10["n"]
    B = pn.dense_of(pn.polynomial(f, two["coef"], two["ks"]), n)
    C = P @ np.linalg.solve(Hc, P.T)
    I = np.eye(n)
    Z2 = B + C @ (I - H @ B)
    ref = Z2 + B @ (I - H @ Z2)

    def exact(rhat):                      # scaled residual -> scaled correction: S_c^-1 Hc^-1 S_c^-1
        return np.linalg.solve(Hc, rhat / c.sc) / c.sc
    M = pn.dense_of(pn.two_level_cycle(f, c, t10["P"], two, coarse_solve=exact), n)
    assert relmax(M, ref) < 1e-10


def test_three_level_cycle_nests_the_two_level_form(t10):
    """with the level-3 polynomial inside, the vertex level is itself a textbook cycle: B2, C3 = P2 (poly of H3) P2^T"""
    f, c, l3, _, three = t10_states(t10, 64)
    H, P, Hc, P2 = t10["H"].toarray(), t10["P"].toarray(), t10["Hc"].toarray(), t10["P2"].toarray()
    n, nc = t10["n"], t10["Hc"].shape[0]
    co = three["coef"]
    B = pn.dense_of(pn.polynomial(f, co, three["ks"]), n)
    B2 = pn.dense_of(pn.polynomial(c, co[three["cf_coarse"]:], three["ks2"]), nc)
    Q3 = pn.dense_of(pn.polynomial(l3, co[three["cf_level3"]:], three["k3"]), l3.n)
    C3 = P2 @ Q3 @ P2.T
    I2 = np.eye(nc)
    Y = B2 + C3 @ (I2 - Hc @ B2)
    M2 = Y + B2 @ (I2 - Hc @ Y)
    C = P @ M2 @ P.T
    I = np.eye(n)
    Z2 = B + C @ (I - H @ B)
    ref = Z2 + B @ (I - H @ Z2)
    M = pn.dense_of(pn.three_level_cycle(f, c, l3, t10["P"], t10["P2"], three), n)
    assert relmax(M, ref) < 1e-10


def test_node_block_form_is_the_polynomial_of_the_transformed_matrix(shell):
    H, n = shell["H"].toarray(), shell["n"]
    Linv = np.zeros((n, n))
    for p in range(n // 12):
        s = slice(12 * p, 12 * p + 12)
        Linv[s, s] = np.linalg.inv(np.linalg.cholesky(H[s, s]))
    Hh = Linv @ H @ Linv.T
    w, V = np.linalg.eigh(Hh)
    lam = 1.15 * w.max()
    coef = np.array(pn.chebyshev_pairs(lam, 200.0, 16)).reshape(-1)
    ref = Linv.T @ (V * cheb_q(w, lam, 200.0, 16)) @ V.T @ Linv
    M = pn.dense_of(pn.node_block_form(shell["H"], coef, 16, 64, linv32=False), n)
    assert relmax(M, ref) < 1e-10


def test_float32_work_vectors_and_pcg(t10):
    """the dtype switch moves the result by fp32 round-off only, and the plain PCG reaches the fp64 solution with any
    of the operators in nearly the same number of iterations"""
    rng = np.random.default_rng(3)
    b = rng.normal(size=t10["n"])
    x_ref = np.linalg.solve(t10["H"].toarray(), b)
    its = {}
    for dt in (np.float64, np.float32):
        f, c = pn.Level(t10["H"], 16, dt), pn.Level(t10["Hc"], 16, dt)
        _, _, _, two, _ = t10_states(t10, 16)
        op = pn.two_level_cycle(f, c, t10["P"], two)
        its[dt] = (op(b), pn.pcg(t10["H"], b, op, 1e-12))
    z64, z32 = its[np.float64][0], its[np.float32][0]
    floor = np.linalg.norm(z32 - z64) / np.linalg.norm(z64)
    assert 0.0 < floor < 1e-4, floor
    for dt, (_, (x, it, rel)) in its.items():
        assert rel <= 1e-12 and np.abs(x - x_ref).max() <= 1e-8 * np.abs(x_ref).max(), dt
    assert abs(its[np.float64][1][1] - its[np.float32][1][1]) <= 2, its
