"""The numpy restatement of the shape sensitivities (tests/shape_np.py) against central differences of the CPU oracle's
implicit step over the reference geometry, on the cube mesh, SVK and Mooney-Rivlin.  The problem is that of
tests/test_adjoint_np.py (same step, density, tolerance, random state and cotangents); the oracle is rebuilt with
X +- eps d, so CalcDnDuPre and CalcMassMatrix run again, while x_prev, the targets, the fixed nodes, f_ext and a stay.

Bound: test_adjoint_np's 1e-5 relative per directional derivative, at eps = 1e-4 of the mesh extent."""
import numpy as np
import pytest

from tests import adjoint_np as anp
from tests import shape_np as snp
from tests.test_adjoint_np import BOUND, H_STEP, RHO, Problem

EPS_REL = 1e-4


def loss_at(p, X):
    keep = p.X
    p.X = X
    try:
        return p.loss()
    finally:
        p.X = keep


@pytest.fixture(scope="module", params=["svk", "mr"])
def case(request):
    p = Problem(request.param)
    model = "mr" if p.kind == "mr" else "svk"
    o, x, v, _ = p.step()
    ro, ci, val = o.assemble_hessian(H_STEP, RHO)
    n = 3 * p.N
    H = np.zeros((n, n))
    for r in range(n):
        H[r, ci[ro[r]:ro[r + 1]]] += val[ro[r]:ro[r + 1]]
    H = np.triu(H) + np.triu(H, 1).T if np.allclose(np.tril(H, -1), 0.0) else H
    J = anp.selector_J(p.fixed, p.N)
    w, out = anp.adjoint_step(H, o.m_off, o.m_col, o.m_val, J, H_STEP, RHO, p.xbar, p.vbar, p.lambar)
    gradN = o.gradN_a_d()
    F = anp.deformation_gradients(x.reshape(-1, 3), p.conn, gradN)
    Nq = anp.shape_values(o.qx, o.qy, o.qz)
    u = (v - p.v_prev) / H_STEP - np.tile(p.a, p.N)
    L = np.ptp(p.X, axis=0).max()
    rng = np.random.default_rng(23)
    dirs = [rng.normal(size=p.X.shape) for _ in range(3)]  # every node moves, the mid-edge nodes on their own
    eps = EPS_REL * L
    fd = [(loss_at(p, p.X + eps * d / np.abs(d).max()) - loss_at(p, p.X - eps * d / np.abs(d).max())) /
          (2.0 * eps / np.abs(d).max()) for d in dirs]

    def restated(**kw):
        rows = snp.shape_rows(F, None, gradN, o.detJ, o.qw, p.conn, w, u, Nq, model, p.theta, p.rho0, **kw)
        return snp.scatter(rows, p.conn, p.N)
    return dict(p=p, o=o, model=model, F=F, w=w, out=out, dirs=dirs, fd=fd, restated=restated, gradN=gradN)


def gaps(Xbar, case):
    return [abs(float(np.sum(Xbar * d)) - f) / abs(f) for d, f in zip(case["dirs"], case["fd"])]


def test_shape_cotangent_matches_central_differences(case):
    g = gaps(case["restated"](), case)
    for k, v in enumerate(g):
        print(f"{case['p'].kind} direction {k}: relative gap {v:.3e}")
    assert all(v <= BOUND for v in g), g


def test_per_element_parameters_give_the_same_rows(case):
    """theta [E, P] and rho [E] (material tables) are the uniform values spelled out"""
    p, o = case["p"], case["o"]
    E = p.conn.shape[0]
    Nq = anp.shape_values(o.qx, o.qy, o.qz)
    u = np.linspace(-1.0, 1.0, 3 * p.N)
    args = (case["F"], None, case["gradN"], o.detJ, o.qw, p.conn, case["w"], u, Nq, case["model"])
    a = snp.shape_rows(*args, p.theta, p.rho0)
    b = snp.shape_rows(*args, np.tile(p.theta, (E, 1)), np.full(E, p.rho0))
    assert np.array_equal(a, b)


def test_closed_form_tangent_against_central_differences_of_P(case):
    """dP[D] closed form against (P(F + t D) - P(F - t D)) / 2t, t = 1e-6 / max|D|: truncation ~ t^2 |P'''| / 6 and
    rounding ~ 1e-16 |P| / t, both relative to |dP[D]|.
    Measured gap: SVK 2.0e-10, Mooney-Rivlin 2.9e-10 -> bound 100 x the larger = 2.9e-8 (no looser than 1e-6)."""
    p = case["p"]
    F = case["F"]
    rng = np.random.default_rng(5)
    D = rng.normal(size=F.shape)
    t = 1e-6 / np.abs(D).max()
    fd = (snp.stress_P(F + t * D, case["model"], p.theta) - snp.stress_P(F - t * D, case["model"], p.theta)) / (2.0 * t)
    cf = snp.dP_D(F, D, case["model"], p.theta)
    gap = float(np.abs(cf - fd).max() / np.abs(fd).max())
    print(f"{p.kind}: closed-form dP[D] against central differences of P: relative gap {gap:.3e}")
    assert gap <= 2.9e-8


@pytest.mark.parametrize("mistake", [dict(drop_DtP=True), dict(drop_FtdP=True), dict(drop_mass=True), dict(sign=-1.0)])
def test_the_check_catches_a_wrong_restatement(case, mistake):
    g = gaps(case["restated"](**mistake), case)
    print(case["p"].kind, mistake, g)
    assert all(v > BOUND for v in g), g


def test_rigid_translation_identity(case):
    """Moving X, x_prev and the targets by one vector c leaves g unchanged and v with it; x moves by c and lambda_new stays.
    So the loss moves by sum_b xbar_b . c, and that is what the three cotangents must add up to:
        sum_b X_bar_b + sum_b x_prev_bar_b + sum_k t_bar_k - sum_b xbar_b = 0
    to rounding.  The identity holds for any w (it is g's invariance), so no solve error enters: the sums are of ~N
    fp64 terms, bounded by 1e-13 x the sum of their magnitudes (N ~ 1e2 .. 1e3 roundings of 1.1e-16)."""
    p, out = case["p"], case["out"]
    parts = [case["restated"](), out["x_prev"].reshape(-1, 3), out["targets"].reshape(-1, 3), -p.xbar.reshape(-1, 3)]
    total = sum(a.sum(axis=0) for a in parts)
    mag = sum(np.abs(a).sum(axis=0) for a in parts)
    largest = max(np.abs(a).max() for a in parts)
    print(f"{p.kind}: translation sum {total}, relative to the largest term {np.abs(total).max() / largest:.3e}, "
          f"to the sum of magnitudes {np.abs(total / mag).max():.3e}")
    assert np.all(np.abs(total) <= 1e-13 * mag)
