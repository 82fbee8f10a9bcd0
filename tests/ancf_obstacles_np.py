"""NumPy restatement of the rigid-obstacle contact of the ANCF kinds (DESIGN 3e'): the 32 sample points of an element and
their weights, the shape values from the monomial basis and the matrix B of the nodal conditions, the per-point model of
tests/obstacles_np.py, and dense assembly of the contact force and Hessian.  Problems are the tuples of
tests/ancf_stress_np.py: (kind, x12, y12, z12, conn_nodes, (L, W, H))."""
import numpy as np

from tests import obstacles_np as onp

# monomials u^a v^b w^c of the two elements (beam: cubic along u, linear across; shell: bicubic-incomplete in u, v)
EXP = {3243: np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [2, 0, 0], [3, 0, 0]]),
       3443: np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1], [2, 0, 0],
                       [0, 2, 0], [2, 1, 0], [1, 2, 0], [3, 0, 0], [0, 3, 0], [3, 1, 0], [1, 3, 0]])}
NODES = {3243: np.array([[-1, 0, 0], [1, 0, 0]]), 3443: np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]])}
G4, W4 = np.polynomial.legendre.leggauss(4)
G2, W2 = np.polynomial.legendre.leggauss(2)
P = 32


def basis(kind, u, which=0):
    """monomials at u = (u, v, w) (which = 0) or their derivative along axis which - 1"""
    ex = EXP[kind]
    if which == 0:
        return np.prod(np.power(u[None, :], ex), axis=1)
    d = which - 1
    lo = ex.copy()
    lo[:, d] = np.maximum(lo[:, d] - 1, 0)
    return ex[:, d] * np.prod(np.power(u[None, :], lo), axis=1)


def B_matrix(kind, L, W):
    """rows: (b, b_u, b_v, b_w) at every node of the element, node after node"""
    half = np.array([L / 2, W / 2, 0.0])
    return np.array([basis(kind, n * half, which) for n in NODES[kind] for which in range(4)])


def sample_points(kind):
    """[(xi, eta, zeta, quadrature weight, the two directions that span the face)] in the kernels' point order"""
    pts = []
    if kind == 3443:
        for zeta in (-1.0, 1.0):
            pts += [(G4[i], G4[j], zeta, W4[i] * W4[j], 0, 1) for i in range(4) for j in range(4)]
    else:
        for eta in (-1.0, 1.0):
            pts += [(G4[i], eta, G2[k], W4[i] * W2[k], 0, 2) for i in range(4) for k in range(2)]
        for zeta in (-1.0, 1.0):
            pts += [(G4[i], G2[k], zeta, W4[i] * W2[k], 0, 1) for i in range(4) for k in range(2)]
    return pts


def shape_values(kind, dims, which=0):
    """[32, S]: S_a(p) = ((B^T)^-1 b(p))_a, or its derivative along the normalised coordinate which - 1"""
    L, W, H = dims
    half = np.array([L / 2, W / 2, H / 2])
    BT = B_matrix(kind, L, W).T
    rows = []
    for xi, eta, zeta, *_ in sample_points(kind):
        b = basis(kind, np.array([xi, eta, zeta]) * half, which)
        rows.append(np.linalg.solve(BT, b) * (half[which - 1] if which else 1.0))
    return np.array(rows)


def coef_ids(prob):
    """[E, S] coefficient ids: 4 node + slot, node after node"""
    conn = np.asarray(prob[4])
    return (4 * conn[:, :, None] + np.arange(4)[None, None, :]).reshape(conn.shape[0], -1)


def reference(prob):
    return np.stack(prob[1:4], axis=1)


def weights(prob):
    """[E, 32]: quadrature weight x |r_a x r_b| of the reference configuration, a, b the face's two directions"""
    kind, dims = prob[0], prob[5]
    X = reference(prob)[coef_ids(prob)]                                  # [E, S, 3]
    dS = [shape_values(kind, dims, which) for which in (1, 2, 3)]         # d/dxi, d/deta, d/dzeta
    pts = sample_points(kind)
    w = np.zeros((X.shape[0], P))
    for p, (_, _, _, qw, a, b) in enumerate(pts):
        ta = np.einsum("s,esc->ec", dS[a][p], X)
        tb = np.einsum("s,esc->ec", dS[b][p], X)
        w[:, p] = qw * np.linalg.norm(np.cross(ta, tb), axis=1)
    return w


def positions(prob, x):
    """[E, 32, 3] sample points at the coefficient vectors x [n_coef, 3]"""
    return np.einsum("ps,esc->epc", shape_values(prob[0], prob[5]), np.asarray(x)[coef_ids(prob)])


def energy(prob, obstacles, x, xp, h):
    r, r0, w = positions(prob, x), positions(prob, xp), weights(prob)
    return sum(onp.energy(o, w[e, p], r[e, p], r0[e, p], h) for e in range(r.shape[0]) for p in range(P) for o in obstacles)


def assemble(prob, obstacles, x, xp, h):
    """dict: force [n_coef, 3], hessian [3 n_coef, 3 n_coef] (h x the blocks, the solver's scaling), per point the force
    fp [E, 32, 3] and block Cp [E, 32, 3, 3], gap and pressure [E, 32], touched [E], per obstacle (resultant, points in
    contact), and `curvature`: the sphere term kappa w d (I - n n^T) / |r| that the Gauss-Newton block leaves out."""
    kind, dims = prob[0], prob[5]
    ids, Sv, w = coef_ids(prob), shape_values(kind, dims), weights(prob)
    r, r0 = positions(prob, x), positions(prob, xp)
    E, n = ids.shape[0], np.asarray(x).shape[0]
    fp, Cp, cur = np.zeros((E, P, 3)), np.zeros((E, P, 3, 3)), np.zeros((E, P, 3, 3))
    gap, press = np.full((E, P), np.inf), np.zeros((E, P))
    touched = np.zeros(E, dtype=bool)
    res = [[np.zeros(3), 0] for _ in obstacles]
    for e in range(E):
        for p in range(P):
            for k, o in enumerate(obstacles):
                f, b = onp.force_block(o, w[e, p], r[e, p], r0[e, p], h)
                d, nrm = onp.distance(o, r[e, p])
                fp[e, p] += f
                Cp[e, p] += b
                res[k][0] += f
                res[k][1] += int(d < 0)
                gap[e, p] = min(gap[e, p], d)
                press[e, p] += o["kappa"] * max(-d, 0.0)
                touched[e] |= d < 0 or (o["mu"] > 0 and onp.distance(o, r0[e, p])[0] < 0)
                if d < 0 and o["kind"] == 1:
                    cur[e, p] += o["kappa"] * w[e, p] * d * (np.eye(3) - np.outer(nrm, nrm)) / (d + o["radius"])
    F, Hd, Hc = np.zeros((n, 3)), np.zeros((3 * n, 3 * n)), np.zeros((3 * n, 3 * n))
    for e in range(E):
        np.add.at(F, ids[e], Sv.T @ fp[e])
        for M, blocks in ((Hd, Cp[e]), (Hc, cur[e])):
            K = h * np.einsum("pi,pj,pab->iajb", Sv, Sv, blocks).reshape(3 * Sv.shape[1], -1)
            dof = (3 * ids[e][:, None] + np.arange(3)[None, :]).reshape(-1)
            M[np.ix_(dof, dof)] += K
    return dict(force=F, hessian=Hd, curvature=Hc, fp=fp, Cp=Cp, gap=gap, pressure=press, touched=touched,
                resultants=[(a, c) for a, c in res], weights=w, points=r)
