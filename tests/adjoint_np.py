"""fp64 numpy restatement of the adjoint of the implicit Newton step.

One Solve() with max_outer = 1 finds v with
    g(v) = M (v - v_prev)/h + f_int(x) - f_ext - M a + h J^T (lam + rho (J x - t)) = 0,   x = x_prev + h v,
then lam_new = lam + rho (J x - t).  H = dg/dv is symmetric.  With the cotangents xbar, vbar, lambar of x, v, lam_new:

    xt = xbar + rho J^T lambar      vt = vbar + h xt        solve H w = vt
    f_ext_bar = w                   v_prev_bar = M w / h
    x_prev_bar = xt - (vt - M w / h) / h                    lam_in_bar = lambar - h J w
    t_bar = h rho J w - rho lambar  a_bar = sum_i (M w)_i
    theta_bar[m, p] = - sum_{e in m} sum_q dV_q (dP/dtheta_p)(F_q) : grad w_q
    rho0_bar[m]     = - sum_{e in m} sum_q dV_q (N w)_q . (N u)_q,     u = (v - v_prev)/h - a

Everything works from dense / CSR arrays the caller hands in; nothing here touches a GPU.
"""
import numpy as np

EDGES = [(0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3)]


def shape_values(qx, qy, qz):
    """N [Q, 10]: the T10 shape functions at the rule's points (the mass matrix's rule)"""
    out = np.zeros((len(qx), 10))
    for q in range(len(qx)):
        L = [1.0 - qx[q] - qy[q] - qz[q], qx[q], qy[q], qz[q]]
        for k in range(4):
            out[q, k] = L[k] * (2.0 * L[k] - 1.0)
        for k, (i, j) in enumerate(EDGES):
            out[q, 4 + k] = 4.0 * L[i] * L[j]
    return out


def mass_times(m_off, m_col, m_val, w):
    """(M (x) I3) w for the node-level mass CSR and w [3N]"""
    w3 = np.asarray(w).reshape(-1, 3)
    out = np.zeros_like(w3)
    for i in range(len(m_off) - 1):
        k = slice(m_off[i], m_off[i + 1])
        out[i] = m_val[k] @ w3[m_col[k]]
    return out.reshape(-1)


def selector_J(fixed, N):
    """J [3 n_fixed, 3N] of fixed nodes: constraint 3 k + c is component c of node fixed[k]"""
    J = np.zeros((3 * len(fixed), 3 * N))
    for k, n in enumerate(fixed):
        for c in range(3):
            J[3 * k + c, 3 * n + c] = 1.0
    return J


def csr_J(off, col, val, N):
    J = np.zeros((len(off) - 1, 3 * N))
    for r in range(len(off) - 1):
        for k in range(off[r], off[r + 1]):
            J[r, col[k]] += val[k]
    return J


def rhs_vectors(J, h, rho, xbar, vbar, lambar, drop_jt=False):
    """(xt, vt); drop_jt leaves the rho J^T lambar term out (the mistake the checker must catch)"""
    xt = np.array(xbar, dtype=np.float64)
    if J.shape[0] and not drop_jt:
        xt = xt + rho * (J.T @ lambar)
    return xt, vbar + h * xt


def vector_outputs(w, Mw, J, h, rho, xt, vt, lambar):
    """the five output vectors and a_bar from the adjoint field w and M w"""
    Jw = J @ w if J.shape[0] else np.zeros(0)
    return dict(f_ext=w.copy(), v_prev=Mw / h, x_prev=xt - (vt - Mw / h) / h, lam_in=lambar - h * Jw,
                targets=h * rho * Jw - rho * lambar, gravity=Mw.reshape(-1, 3).sum(axis=0))


def adjoint_step(H, m_off, m_col, m_val, J, h, rho, xbar, vbar, lambar, drop_jt=False, sign=1.0):
    """the vector side from a dense H: -> (w, dict of outputs).  sign = -1 flips f_ext_bar's sign (checker test)."""
    xt, vt = rhs_vectors(J, h, rho, xbar, vbar, lambar, drop_jt)
    w = sign * np.linalg.solve(H, vt)
    return w, vector_outputs(w, mass_times(m_off, m_col, m_val, w), J, h, rho, xt, vt, lambar)


def deformation_gradients(X, conn, gradN):
    """F [E, Q, 3, 3] = sum_a x_a (x) h_a from positions X [N, 3], conn [E, 10], gradN [E, Q, 10, 3]"""
    return np.einsum("eai,eqaj->eqij", X[conn], gradN)


def dP_dtheta(F, model):
    """[P, ..., 3, 3]: derivative of the first Piola-Kirchhoff stress with respect to each stiffness parameter.
    SVK (lambda, mu): tr(E) F, 2 F E.  Mooney-Rivlin (mu10, mu01, kappa) with G = F^-T, C = F^T F:
    2 J^-2/3 (F - I1/3 G), 2 J^-4/3 (I1 F - F C - 2 I2/3 G), (J - 1) J G."""
    C = np.swapaxes(F, -1, -2) @ F
    I = np.eye(3)
    if model == "svk":
        E = 0.5 * (C - I)
        trE = np.trace(E, axis1=-2, axis2=-1)[..., None, None]
        return np.stack([trE * F, 2.0 * F @ E])
    Jd = np.linalg.det(F)[..., None, None]
    G = np.swapaxes(np.linalg.inv(F), -1, -2)
    I1 = np.trace(C, axis1=-2, axis2=-1)[..., None, None]
    I2 = 0.5 * (I1 * I1 - np.trace(C @ C, axis1=-2, axis2=-1)[..., None, None])
    return np.stack([2.0 * Jd ** (-2.0 / 3.0) * (F - I1 / 3.0 * G),
                     2.0 * Jd ** (-4.0 / 3.0) * (I1 * F - F @ C - 2.0 * I2 / 3.0 * G),
                     (Jd - 1.0) * Jd * G])


def sens_per_element(F, gradN, detJ, qw, conn, w, u, model, Nq):
    """[E, P + 1]: the stiffness slots from F directly, then the density slot"""
    w3, u3 = np.asarray(w).reshape(-1, 3), np.asarray(u).reshape(-1, 3)
    dV = detJ * np.asarray(qw)[None, :]
    D = np.einsum("eai,eqaj->eqij", w3[conn], gradN)                  # grad w per point
    dP = dP_dtheta(F, model)                                          # [P, E, Q, 3, 3]
    stiff = -np.einsum("peqij,eqij,eq->ep", dP, D, dV)
    Nw = np.einsum("qa,eai->eqi", Nq, w3[conn])
    Nu = np.einsum("qa,eai->eqi", Nq, u3[conn])
    dens = -np.einsum("eqi,eqi,eq->e", Nw, Nu, dV)
    return np.concatenate([stiff, dens[:, None]], axis=1)


def per_material(pe, ids, n_mat):
    """[n_mat, P + 1]: ascending-element sums per material (ids None: one material)"""
    ids = np.zeros(pe.shape[0], dtype=int) if ids is None else np.asarray(ids)
    return np.stack([pe[ids == m].sum(axis=0) for m in range(n_mat)])
