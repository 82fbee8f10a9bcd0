"""The element map of the matrix-free Hessian product (tests/matfree_np.py) against the oracle's assembled Hessian.

Pins the formula and every scale factor (h, rho0 / h, h^2 rho on pinned rows, the Kelvin-Voigt coefficients) without a
GPU.  Bound: 1e-12 relative to max |y|, the project's bound for H against the oracle (DESIGN 3a'')."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import orc
from tests import matfree_np
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_oracle, perturbed_state

H_STEP, RHO_PEN = 1e-3, 1e14
TOL = 1e-12


def _case(mesh, mat, pinned):
    X, conn = load_mesh(mesh)
    m = MATERIALS[mat]
    fixed = fixed_x0(X) if pinned else None
    o = make_oracle(X, conn, m, fixed)
    x, _ = perturbed_state(X, sigma=2e-2)   # a deformed state: F differs from I by a few per cent
    o.x, o.y, o.z = (np.ascontiguousarray(x[:, i]) for i in range(3))
    ro, ci, val = o.assemble_hessian(H_STEP, RHO_PEN)
    n = 3 * o.N
    H = sp.csr_matrix((val, ci, ro), shape=(n, n))
    quad = orc.keast5()

    def apply(p):
        return matfree_np.apply_hessian(X, conn, x, quad, o.mat.lam, o.mat.mu, o.mat.rho0, H_STEP, p,
                                        eta=o.mat.eta_damp, lamd=o.mat.lambda_damp, fixed=fixed, rho_pen=RHO_PEN)
    return o, H, apply, fixed


@pytest.mark.parametrize("mesh", ["cube", "beam_3x2x1"])
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("mat", ["svk", "svk_damped"])
def test_element_map_equals_assembled_hessian(mesh, pinned, mat):
    o, H, apply, fixed = _case(mesh, mat, pinned)
    if pinned:
        assert len(fixed) > 0
    n = 3 * o.N
    rng = np.random.default_rng(7)
    vecs = [rng.normal(size=n) for _ in range(3)]
    for dof in (0, n // 2, n - 1) + ((3 * int(fixed[0]) + 1,) if pinned else ()):   # unit vectors, a pinned DOF among them
        u = np.zeros(n)
        u[dof] = 1.0
        vecs.append(u)
    for p in vecs:
        y_ref = H @ p
        y = apply(p)
        err = float(np.max(np.abs(y - y_ref)) / np.max(np.abs(y_ref)))
        print(f"{mesh} {mat} pinned={pinned}: max |y - H p| / max |H p| = {err:.3e}")
        assert err < TOL, err


def test_vertex_gradients_match_the_stored_shape_gradients():
    """the affine premise on the test meshes: grad N_j(q) = sum_n c_jn(q) g_n and a constant det J, to rounding"""
    for mesh in ("cube", "beam_3x2x1"):
        X, conn = load_mesh(mesh)
        o = make_oracle(X, conn, MATERIALS["svk"])
        g, detJ = matfree_np.vertex_gradients(X, conn)
        qx, qy, qz, _ = orc.keast5()
        _, c = matfree_np.shape_tables(qx, qy, qz)
        gradN = np.einsum("qjn,end->eqjd", c, g)
        ref = o.gradN_a_d()
        assert np.max(np.abs(gradN - ref)) < 1e-12 * np.max(np.abs(ref))
        assert np.max(np.abs(o.detJ - detJ[:, None])) < 1e-12 * np.max(np.abs(detJ))
