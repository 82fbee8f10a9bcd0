"""NumPy restatement of the distributed loads of the ANCF kinds: the consistent load of a body acceleration
from a mass matrix integrated here, the dead traction on the obstacle sample points of a face, and the follower pressure
on an n x n (shell) or n x m (beam) Gauss rule at the current coefficients.  Problems are the tuples of
tests/ancf_stress_np.py: (kind, x12, y12, z12, conn_nodes, (L, W, H)); faces are numbered as the sample points are
(shell zeta = -1, +1 -> 0, 1; beam eta = -1, +1, zeta = -1, +1 -> 0..3)."""
import numpy as np

from tests import ancf_obstacles_np as aonp
from tests.helpers import tl

Q = tl.quadrature
FACES = {3443: 2, 3243: 4}
RULE = {3443: (5, 5), 3243: (5, 2)}      # the kernels' pressure rule: points along xi, points across


def face_points(kind, face, n_long=None, n_across=None):
    """[(xi, eta, zeta, weight, d0, d1)] Gauss points of a face, the first direction outermost (the kernels' order)"""
    n_long = RULE[kind][0] if n_long is None else n_long
    n_across = RULE[kind][1] if n_across is None else n_across
    g, w = np.polynomial.legendre.leggauss(n_long)
    h, v = np.polynomial.legendre.leggauss(n_across)
    sgn = 1.0 if face & 1 else -1.0
    if kind == 3443:
        return [(g[i], h[j], sgn, w[i] * v[j], 0, 1) for i in range(n_long) for j in range(n_across)]
    if face < 2:
        return [(g[i], sgn, h[k], w[i] * v[k], 0, 2) for i in range(n_long) for k in range(n_across)]
    return [(g[i], h[k], sgn, w[i] * v[k], 0, 1) for i in range(n_long) for k in range(n_across)]


def face_sign(kind, face):
    """s with (outward normal) dA = s (r_d0 x r_d1) d(d0) d(d1): r_xi x r_eta points along +zeta, r_xi x r_zeta along -eta"""
    if kind == 3443:
        return 1.0 if face else -1.0
    return 1.0 if face in (0, 3) else -1.0


def shape_at(kind, dims, pts, which=0):
    """[len(pts), S]: S_a = ((B^T)^-1 b)_a at the points, or its derivative along the normalised coordinate which - 1"""
    L, W, H = dims
    half = np.array([L / 2, W / 2, H / 2])
    BT = aonp.B_matrix(kind, L, W).T
    rows = [np.linalg.solve(BT, aonp.basis(kind, np.array(p[:3]) * half, which)) * (half[which - 1] if which else 1.0)
            for p in pts]
    return np.array(rows)


def pressure_force(prob, x, face, elems, p, n_long=None, n_across=None):
    """[n_coef, 3]: f_a = -p sum_q w_q S_a(q) (outward normal dA)(q) at the coefficients x, on `face` of `elems`"""
    kind, dims = prob[0], prob[5]
    ids = aonp.coef_ids(prob)
    pts = face_points(kind, face, n_long, n_across)
    w = np.array([q[3] for q in pts])
    Sv = shape_at(kind, dims, pts)
    D0, D1 = shape_at(kind, dims, pts, pts[0][4] + 1), shape_at(kind, dims, pts, pts[0][5] + 1)
    x = np.asarray(x)
    F = np.zeros_like(x)
    for e in elems:
        X = x[ids[e]]
        fq = -p * face_sign(kind, face) * w[:, None] * np.cross(D0 @ X, D1 @ X)
        np.add.at(F, ids[e], Sv.T @ fq)
    return F


def face_slice(kind, face):
    ppf = aonp.P // FACES[kind]
    return slice(face * ppf, (face + 1) * ppf)


def traction_force(prob, face, elems, t):
    """[n_coef, 3]: f_a = t sum_p w_p S_a(p) over the obstacle sample points of the face (reference weights)"""
    kind = prob[0]
    ids, Sv, w = aonp.coef_ids(prob), aonp.shape_values(kind, prob[5]), aonp.weights(prob)
    sl = face_slice(kind, face)
    F = np.zeros((len(prob[1]), 3))
    for e in elems:
        np.add.at(F, ids[e], np.outer(Sv[sl].T @ w[e, sl], np.asarray(t, dtype=float)))
    return F


def traction_work(prob, x, face, elems, t):
    """W = int t . r dA over the reference face, by the same points"""
    r, w = aonp.positions(prob, x), aonp.weights(prob)
    sl = face_slice(prob[0], face)
    return float(sum(w[e, sl] @ (r[e, sl] @ np.asarray(t, dtype=float)) for e in elems))


def mass_matrix(prob, rho):
    """dense [n_coef, n_coef] consistent mass: the mass rule of the element kind, det J of the reference map"""
    kind, dims = prob[0], prob[5]
    if kind == 3243:
        rule = (Q.gauss_xi_m_6, Q.gauss_eta_2, Q.gauss_zeta_2, Q.weight_xi_m_6, Q.weight_eta_2, Q.weight_zeta_2)
    else:
        rule = (Q.gauss_xi_m_7, Q.gauss_eta_m_7, Q.gauss_zeta_m_3, Q.weight_xi_m_7, Q.weight_eta_m_7, Q.weight_zeta_m_3)
    gx, gy, gz, wx, wy, wz = (np.asarray(a, dtype=float) for a in rule)
    pts = [(a, b, c, wa * wb * wc) for a, wa in zip(gx, wx) for b, wb in zip(gy, wy) for c, wc in zip(gz, wz)]
    Sv = shape_at(kind, dims, pts)
    dS = [shape_at(kind, dims, pts, which) for which in (1, 2, 3)]
    ids, X = aonp.coef_ids(prob), aonp.reference(prob)
    n = X.shape[0]
    M = np.zeros((n, n))
    for e in range(ids.shape[0]):
        Xe = X[ids[e]]
        J = np.stack([d @ Xe for d in dS], axis=2)                        # [q, i, direction]
        wd = np.array([p[3] for p in pts]) * np.linalg.det(J)
        M[np.ix_(ids[e], ids[e])] += rho * np.einsum("q,qa,qb->ab", wd, Sv, Sv)
    return M


def acceleration_field(n_coef, a):
    """[n_coef, 3]: a on the position coefficients 4 n, 0 on the gradient coefficients"""
    A = np.zeros((n_coef, 3))
    A[0::4] = np.asarray(a, dtype=float)
    return A


def gravity_force(prob, rho, a):
    return mass_matrix(prob, rho) @ acceleration_field(len(prob[1]), a)


def total(prob, x, rho, gravity=None, loads=()):
    """[n_coef, 3] load of a body acceleration and a list of dicts(kind 0 | 1, face, elems, value, scale)"""
    F = np.zeros((len(prob[1]), 3))
    if gravity is not None:
        F += gravity_force(prob, rho, gravity)
    for ld in loads:
        if ld["kind"] == 0:
            F += ld["scale"] * traction_force(prob, ld["face"], ld["elems"], ld["value"])
        else:
            F += pressure_force(prob, x, ld["face"], ld["elems"], ld["scale"] * ld["value"])
    return F


def field_on(big, x_big, fine):
    """Coefficients of the mesh `fine` that carry the polynomial field of the one-element problem `big` at x_big (both on
    the same rectangle / line, element axes along the global ones): r, r_u, r_v, r_w of the field at every node of `fine`.
    The monomial spaces of both kinds are closed under translation, so the refined mesh represents the field exactly."""
    kind, (L, W, H) = big[0], big[5]
    Xb, Xf = aonp.reference(big), aonp.reference(fine)
    Xe = np.asarray(x_big)[aonp.coef_ids(big)[0]]
    lo = Xb[0::4].min(axis=0)
    out = np.zeros_like(Xf)
    for n in range(Xf.shape[0] // 4):
        P = Xf[4 * n]
        pt = [(2 * (P[0] - lo[0]) / L - 1.0, 2 * (P[1] - lo[1]) / W - 1.0 if kind == 3443 else 0.0, 0.0)]
        out[4 * n] = shape_at(kind, big[5], pt)[0] @ Xe
        for d, half in enumerate((L / 2, W / 2, H / 2)):
            out[4 * n + 1 + d] = shape_at(kind, big[5], pt, d + 1)[0] @ Xe / half
    return out
