"""fp64 numpy restatement of the shape sensitivities of the implicit Newton step.

With the adjoint field w of tests/adjoint_np.py (H w = vt) and u = (v - v_prev)/h - a, the cotangent of the reference
coordinates X of all ten nodes of every element is X_bar = - w . dg/dX.  Per quadrature point, with G_b = grad_X N_b,
F = sum_a x_a (x) G_a, D = sum_a w_a (x) G_a, dV = w_q det J, a variation dX gives L = dX^T G and
    dG = -G L,  dF = -F L,  dD = -D L,  d(dV) = dV tr L,
so that, the material tangent being symmetric,
    S_q   = (P : D + rho Nw . Nu) I - F^T dP[D] - D^T P
    X_bar = - sum_{e, q} dV_q S_q G_b,q          (row of node b)
dP[D] = (dP/dF) : D in closed form for both models.  Nothing here touches a GPU.
"""
import numpy as np

from tests import adjoint_np as anp

I3 = np.eye(3)


def _t(A):
    return np.swapaxes(A, -1, -2)


def _tr(A):
    return np.trace(A, axis1=-2, axis2=-1)[..., None, None]


def _dd(A, B):
    return np.sum(A * B, axis=(-2, -1))[..., None, None]


def _theta(theta, F):
    """parameter p of theta ([P] or per element [E, P]) shaped to broadcast against F [E, Q, 3, 3] (or [..., 3, 3])"""
    th = np.asarray(theta, dtype=np.float64)
    if th.ndim == 1:
        return [th[p] for p in range(len(th))]
    return [th[:, p].reshape((-1,) + (1,) * (F.ndim - 1)) for p in range(th.shape[1])]


def stress_P(F, model, theta):
    """first Piola-Kirchhoff stress: P is linear in its stiffness parameters (adjoint_np.dP_dtheta)"""
    return sum(t * d for t, d in zip(_theta(theta, F), anp.dP_dtheta(F, model)))


def dP_D(F, D, model, theta):
    """the material tangent of P applied to D, closed form.
    SVK: D S2 + F (lambda tr(dE) I + 2 mu dE), dE = sym(F^T D), S2 = lambda tr(E) I + 2 mu E.
    Mooney-Rivlin, term by term of adjoint_np.dP_dtheta, with g = G : D (dJ = J g), dI1 = 2 F : D, dC = F^T D + D^T F,
    dI2 = I1 dI1 - tr(C dC), dG = -G D^T G."""
    th = _theta(theta, F)
    C = _t(F) @ F
    if model == "svk":
        lam, mu = th
        E = 0.5 * (C - I3)
        dE = 0.5 * (_t(F) @ D + _t(D) @ F)
        S2 = lam * _tr(E) * I3 + 2.0 * mu * E
        return D @ S2 + F @ (lam * _tr(dE) * I3 + 2.0 * mu * dE)
    mu10, mu01, kappa = th
    J = np.linalg.det(F)[..., None, None]
    G = _t(np.linalg.inv(F))
    I1 = _tr(C)
    I2 = 0.5 * (I1 * I1 - _tr(C @ C))
    g = _dd(G, D)
    dI1 = 2.0 * _dd(F, D)
    dC = _t(F) @ D + _t(D) @ F
    dI2 = I1 * dI1 - _tr(C @ dC)
    dG = -G @ _t(D) @ G
    a1, a2 = 2.0 * J ** (-2.0 / 3.0), 2.0 * J ** (-4.0 / 3.0)
    T1 = F - I1 / 3.0 * G
    T2 = I1 * F - F @ C - 2.0 * I2 / 3.0 * G
    d1 = a1 * (-2.0 / 3.0 * g * T1 + D - dI1 / 3.0 * G - I1 / 3.0 * dG)
    d2 = a2 * (-4.0 / 3.0 * g * T2 + dI1 * F + I1 * D - D @ C - F @ dC - 2.0 * dI2 / 3.0 * G - 2.0 * I2 / 3.0 * dG)
    d3 = (2.0 * J - 1.0) * J * g * G + (J - 1.0) * J * dG
    return mu10 * d1 + mu01 * d2 + kappa * d3


def shape_rows(F, D, gradN, detJ, qw, conn, w, u, Nq, model, theta, rho, drop_DtP=False, drop_FtdP=False,
               drop_mass=False, sign=1.0):
    """per-element rows [E, 10, 3]: sum_q dV_q S_q G_b,q.  F, D [E, Q, 3, 3] (D None: formed from w), gradN
    [E, Q, 10, 3], detJ [E, Q], theta [P] or [E, P], rho a number or [E]; u None: no mass term.  The drop_* / sign
    switches are the mistakes the checker must catch."""
    w3 = np.asarray(w, dtype=np.float64).reshape(-1, 3)
    if D is None:
        D = np.einsum("eai,eqaj->eqij", w3[conn], gradN)
    dV = detJ * np.asarray(qw)[None, :]
    P = stress_P(F, model, theta)
    s = _dd(P, D)[..., 0, 0]
    if u is not None and not drop_mass:
        u3 = np.asarray(u, dtype=np.float64).reshape(-1, 3)
        Nw = np.einsum("qa,eai->eqi", Nq, w3[conn])
        Nu = np.einsum("qa,eai->eqi", Nq, u3[conn])
        s = s + np.asarray(rho, dtype=np.float64).reshape(-1, 1) * np.einsum("eqi,eqi->eq", Nw, Nu)
    S = s[..., None, None] * I3
    if not drop_FtdP:
        S = S - _t(F) @ dP_D(F, D, model, theta)
    if not drop_DtP:
        S = S - _t(D) @ P
    return sign * np.einsum("eq,eqij,eqbj->ebi", dV, S, gradN)


def scatter(rows, conn, N):
    """X_bar [N, 3] = - the sum of every node's element rows"""
    out = np.zeros((N, 3))
    np.add.at(out, conn.reshape(-1), -rows.reshape(-1, 3))
    return out


def straight_sided(Xv, conn):
    """all-node coordinates of a mesh whose mid-edge nodes are the means of their vertices; Xv [N, 3], of which only the
    vertex rows are read"""
    X = np.array(Xv, dtype=np.float64)
    for k, (i, j) in enumerate(anp.EDGES):
        X[conn[:, 4 + k]] = 0.5 * (Xv[conn[:, i]] + Xv[conn[:, j]])
    return X
