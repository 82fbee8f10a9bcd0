"""fp64 numpy restatement of the adjoint of the implicit Newton step on ANCF beams and shells (DESIGN 3j').

The step is that of tests/adjoint_np.py over the n_coef coefficient vectors (positions and gradients alike):
    g(v) = M (v - v_prev)/h + f_int(x) - f_ext - M a^ + h J^T (lam + rho (J x - t)) = 0,   x = x_prev + h v.
What is generic comes from tests/adjoint_np.py (rhs_vectors, vector_outputs, dP_dtheta, csr_J, selector_J, mass_times);
what the ANCF kinds add is here:

    a^_i = a on position coefficients (i % 4 == 0), 0 on gradient coefficients  (body_force_kernel with stride 4)
    u = (v - v_prev)/h - a^         a_bar = sum_{i % 4 == 0} (M w)_i
    theta_bar[p] = - sum_e sum_q dV_q (dP/dtheta_p)(F_q) : D_q,   F = sum_a x_a (x) grad s_a,  D = sum_a w_a (x) grad s_a
                   at the Q force-quadrature points, dV = detJ[e, q] qw[q], gradients from the oracle's gradN [E][Q][3][S]
    rho0_bar     = - (M w) . u / rho0   (M is linear in the object's one density and integrated with its own rule)

The keyword arguments named after mistakes restate the step wrongly on purpose; tests/test_ancf_adjoint_np.py checks that
each of them misses the bound.  Nothing here touches a GPU.
"""
import numpy as np

from tests import adjoint_np as tnp
from tests import ancf_stress_np as anp

STRIDE = 4   # coefficient vectors per mesh node: r, r_u, r_v, r_w


def a_hat(a, n_coef):
    """[3 n_coef]: the body acceleration on the position coefficients, zero on the gradient coefficients"""
    out = np.zeros((n_coef, 3))
    out[0::STRIDE] = np.asarray(a, dtype=np.float64)
    return out.reshape(-1)


def u_vector(v, v_prev, h, a, without_a=False):
    """u = (v - v_prev)/h - a^; without_a leaves the acceleration out (a mistake the checker must catch)"""
    u = (np.asarray(v) - np.asarray(v_prev)) / h
    return u if without_a else u - a_hat(a, len(u) // 3)


def gravity_bar(Mw, all_coefficients=False):
    """a_bar [3]: M w summed over the position coefficients; all_coefficients sums every row (a mistake)"""
    rows = np.asarray(Mw).reshape(-1, 3)
    return rows.sum(axis=0) if all_coefficients else rows[0::STRIDE].sum(axis=0)


def density_bar(Mw, u, rho0, without_division=False):
    """rho0_bar = -(M w) . u / rho0; without_division forgets that M carries the density (a mistake)"""
    s = -float(np.dot(Mw, u))
    return s if without_division else s / rho0


def sens_per_element(o, x, w, model):
    """[E, P]: the stiffness slots at the coefficients x [n_coef, 3] for the adjoint field w [3 n_coef]"""
    F = anp.deformation(o, x)
    D = anp.deformation(o, np.asarray(w).reshape(-1, 3))
    dV = o.detJ * o.qw[None, :]
    return -np.einsum("peqij,eqij,eq->ep", tnp.dP_dtheta(F, model), D, dV)


def dense_H(ro, ci, val, n):
    """dense symmetric H from the oracle's DOF-level CSR (which may hold the upper triangle alone)"""
    H = np.zeros((n, n))
    for r in range(n):
        np.add.at(H[r], ci[ro[r]:ro[r + 1]], val[ro[r]:ro[r + 1]])
    return np.triu(H) + np.triu(H, 1).T if np.allclose(np.tril(H, -1), 0.0) else H


def adjoint_outputs(w, Mw, J, h, rho, xt, vt, lambar, u, rho0, all_coefficients=False, without_division=False):
    """every vector output, a_bar over the position coefficients and the density slot, from w and M w"""
    out = tnp.vector_outputs(w, Mw, J, h, rho, xt, vt, lambar)
    out["gravity"] = gravity_bar(Mw, all_coefficients)
    out["rho0"] = density_bar(Mw, u, rho0, without_division)
    return out


def adjoint_step(H, o, J, h, rho, xbar, vbar, lambar, u, rho0, sign=1.0, drop_jt=False, **mistakes):
    """the vector side from a dense H and the oracle's mass CSR -> (w, outputs).  sign = -1 flips w, drop_jt leaves
    rho J^T lambar out of x_t (both mistakes)."""
    xt, vt = tnp.rhs_vectors(J, h, rho, xbar, vbar, lambar, drop_jt)
    w = sign * np.linalg.solve(H, vt)
    Mw = tnp.mass_times(o.m_off, o.m_col, o.m_val, w)
    return w, adjoint_outputs(w, Mw, J, h, rho, xt, vt, lambar, u, rho0, **mistakes)
