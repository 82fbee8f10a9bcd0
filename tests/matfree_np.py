"""NumPy statement of the matrix-free Hessian product on straight-sided T10 elements with St.Venant-Kirchhoff
(+ Kelvin-Voigt): y = H p formed element by element from the four vertex gradients g_n = grad L_n, det J and F at the
five Keast points -- the linear map that assemble_affine_kernel assembles (DESIGN 3a', 3g).

    dF(q) = sum_j p_j (x) grad N_j(q),    grad N_j(q) = sum_n c_jn(q) g_n
    dE = sym(F^T dF),  dS = a tr(dE) I + 2 b dE,  dP = dF S_h + F dS
        a = h lambda + lamd,  b = h mu + eta,  S_h = h (lambda tr(E) I + 2 mu E)
    y_i = sum_q w_q det J dP(q) grad N_i(q) + (rho0 / h) det J sum_q w_q N_i(q) sum_j N_j(q) p_j
    pinned rows: + h^2 rho p on the diagonal
"""
import numpy as np

EDGES = ((0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3))  # local nodes 4..9


def vertex_gradients(X, conn):
    """g [E,4,3] = grad L_n and det J [E] of the straight-sided element spanned by its four vertices."""
    V = X[conn[:, :4]]                                   # [E,4,3]
    J = (V[:, 1:] - V[:, :1]).transpose(0, 2, 1)         # columns X_k - X_0
    Jinv = np.linalg.inv(J)                              # rows = grad xi_k
    g = np.empty((conn.shape[0], 4, 3))
    g[:, 1:] = Jinv
    g[:, 0] = -Jinv.sum(axis=1)
    return g, np.linalg.det(J)


def shape_tables(qx, qy, qz):
    """N [Q,10] and c [Q,10,4] with grad N_j(q) = sum_n c[q,j,n] g_n."""
    Q = len(qx)
    L = np.stack([1.0 - qx - qy - qz, qx, qy, qz], axis=1)
    N = np.zeros((Q, 10))
    c = np.zeros((Q, 10, 4))
    for k in range(4):
        N[:, k] = L[:, k] * (2.0 * L[:, k] - 1.0)
        c[:, k, k] = 4.0 * L[:, k] - 1.0
    for k, (a, b) in enumerate(EDGES):
        N[:, 4 + k] = 4.0 * L[:, a] * L[:, b]
        c[:, 4 + k, a] = 4.0 * L[:, b]
        c[:, 4 + k, b] = 4.0 * L[:, a]
    return N, c


def apply_hessian(X, conn, x, quad, lam, mu, rho0, h, p, eta=0.0, lamd=0.0, fixed=None, rho_pen=0.0):
    """y = H p.  X reference nodes [N,3], x current nodes [N,3], quad = (qx, qy, qz, qw), p [3N]."""
    qx, qy, qz, qw = quad
    g, detJ = vertex_gradients(X, conn)
    Nq, c = shape_tables(qx, qy, qz)
    gradN = np.einsum("qjn,end->eqjd", c, g)             # [E,Q,10,3]
    xe, pe = x[conn], p.reshape(-1, 3)[conn]             # [E,10,3]
    F = np.einsum("eji,eqjd->eqid", xe, gradN)
    dF = np.einsum("eji,eqjd->eqid", pe, gradN)
    I = np.eye(3)
    C = np.einsum("eqki,eqkj->eqij", F, F)
    Eg = 0.5 * (C - I)
    Sh = h * (lam * np.trace(Eg, axis1=2, axis2=3)[..., None, None] * I + 2.0 * mu * Eg)
    G = np.einsum("eqki,eqkj->eqij", F, dF)
    dE = 0.5 * (G + G.transpose(0, 1, 3, 2))
    dS = (h * lam + lamd) * np.trace(dE, axis1=2, axis2=3)[..., None, None] * I + 2.0 * (h * mu + eta) * dE
    dP = np.einsum("eqik,eqkj->eqij", dF, Sh) + np.einsum("eqik,eqkj->eqij", F, dS)
    dV = detJ[:, None] * qw[None, :]
    ye = np.einsum("eq,eqid,eqjd->eji", dV, dP, gradN)
    ye += (rho0 / h) * np.einsum("eq,qi,qj,ejd->eid", dV, Nq, Nq, pe)
    y = np.zeros((X.shape[0], 3))
    np.add.at(y, conn, ye)
    y = y.reshape(-1)
    if fixed is not None and len(fixed):
        dof = (3 * np.asarray(fixed)[:, None] + np.arange(3)[None, :]).reshape(-1)
        y[dof] += h * h * rho_pen * p[dof]
    return y
