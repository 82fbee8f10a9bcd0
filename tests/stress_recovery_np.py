"""NumPy restatement of the recovered stress (DESIGN 3f''): the extrapolation table, the recovered nodal stress, the
principal stresses and the ZZ error indicator, from point stresses [E][5][6], det J, the weights, the connectivity and
the small-strain moduli of every element.  The `edges`, `weighted` and `table` arguments exist so that the tests can
inject the faults the exactness check must catch."""
import numpy as np

from tests import stress_np as snp

EDGES = ((0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3))  # local order of the mid-edge nodes


def table(bary, edges=EDGES):
    """T [10][5]: the unweighted least-squares fit, linear in the reference coordinates, of the five point values,
    evaluated at the four vertices (pinv of the points' barycentric coordinates) and at the mid-edge nodes."""
    Tv = np.linalg.pinv(np.asarray(bary, dtype=np.float64))   # [4][5]
    return np.vstack([Tv] + [0.5 * (Tv[a] + Tv[b])[None] for a, b in edges])


def shape_at_points(bary, edges=EDGES):
    """Nq [5][10]: the quadratic shape functions at the rule's points."""
    L = np.asarray(bary, dtype=np.float64)
    return np.hstack([L * (2.0 * L - 1.0)] + [(4.0 * L[:, a] * L[:, b])[:, None] for a, b in edges])


def recovered_nodal(points, detJ, qw, conn, n_nodes, T, weighted=True):
    """sigma*_i = sum_e V_e (T[a(e,i)] . sigma_e) / sum_e V_e (weighted = False: the plain mean, a fault)."""
    Ve = (detJ * np.asarray(qw)[None, :]).sum(axis=1)
    w = Ve if weighted else np.ones_like(Ve)
    ext = np.einsum("aq,eqc->eac", T, points)              # [E][10][6]
    num, den = np.zeros((n_nodes, 6)), np.zeros(n_nodes)
    for a in range(conn.shape[1]):                         # add.at adds the elements in ascending order
        np.add.at(num, conn[:, a], w[:, None] * ext[:, a])
        np.add.at(den, conn[:, a], w)
    return num / np.where(den > 0, den, 1.0)[:, None]


def moduli(m):
    """Small-strain (mu, K) of a helpers.MATERIALS-style record."""
    if m["kind"] == "svk":
        lam, mu = snp.lame(m)
        return mu, lam + 2.0 * mu / 3.0
    return 2.0 * (m["mu10"] + m["mu01"]), m["kappa"]


def cinv_norm2(s, mu, K):
    """|s|^2 = dev(s):dev(s) / (2 mu) + tr(s)^2 / (9 K) of 6-vectors xx yy zz xy yz zx."""
    tr = s[..., 0] + s[..., 1] + s[..., 2]
    d = s[..., :3] - tr[..., None] / 3.0
    dd = (d * d).sum(axis=-1) + 2.0 * (s[..., 3:] ** 2).sum(axis=-1)
    return dd / (2.0 * mu) + tr * tr / (9.0 * K)


def error_indicator(points, nodal, detJ, qw, conn, Nq, mu, K):
    """mu, K: scalars or [E].  -> dict(eta2 [E] clamped at 0, n2 [E], eta2_total, n2_total, eta_rel, clamped)."""
    mu, K = np.broadcast_to(mu, detJ.shape[:1])[:, None], np.broadcast_to(K, detJ.shape[:1])[:, None]
    dV = detJ * np.asarray(qw)[None, :]
    eq = np.einsum("qa,eac->eqc", Nq, nodal[conn]) - points
    raw = (dV * cinv_norm2(eq, mu, K)).sum(axis=1)
    eta2, n2 = np.maximum(raw, 0.0), (dV * cinv_norm2(points, mu, K)).sum(axis=1)
    e, n = float(eta2.sum()), float(n2.sum())
    return dict(eta2=eta2, n2=n2, eta2_total=e, n2_total=n, eta_rel=np.sqrt(e / (n + e)) if n + e > 0 else 0.0,
                clamped=int((raw < 0).sum()))


def principal(s6):
    """-> values [..., 3] descending, tau_max, vectors [..., 3, 3] (rows, numpy's, not made right-handed)."""
    w, v = np.linalg.eigh(snp.tensor(np.asarray(s6, dtype=np.float64)))
    return w[..., ::-1], 0.5 * (w[..., 2] - w[..., 0]), np.swapaxes(v, -1, -2)[..., ::-1, :]


def element_mean(points, detJ, qw):
    dV = detJ * np.asarray(qw)[None, :]
    return np.einsum("eq,eqc->ec", dV, points) / dV.sum(axis=1)[:, None]


def todays_nodal(points, detJ, qw, conn, n_nodes):
    """The nodal stress of DESIGN 3f: the V_e-weighted mean of the element mean stresses."""
    Ve = (detJ * np.asarray(qw)[None, :]).sum(axis=1)
    es = element_mean(points, detJ, qw)
    num, den = np.zeros((n_nodes, 6)), np.zeros(n_nodes)
    for a in range(conn.shape[1]):
        np.add.at(num, conn[:, a], Ve[:, None] * es)
        np.add.at(den, conn[:, a], Ve)
    return num / np.where(den > 0, den, 1.0)[:, None]


# ---- the smooth imposed field of the convergence study: x = X + a u(X) ---------------------------------------------------
SMOOTH_A = 0.02


def smooth_position(X, a=SMOOTH_A):
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    u = np.stack([np.sin(1.3 * x) * y, np.cos(0.9 * x + z), np.sin(1.1 * x) * np.cos(y) + 0.3 * x * x], axis=-1)
    return X + a * u


def smooth_gradient(X, a=SMOOTH_A):
    """F = I + a du/dX, analytic, [..., 3, 3]."""
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    o = np.zeros_like(x)
    G = np.stack([np.stack([1.3 * np.cos(1.3 * x) * y, np.sin(1.3 * x), o], axis=-1),
                  np.stack([-0.9 * np.sin(0.9 * x + z), o, -np.sin(0.9 * x + z)], axis=-1),
                  np.stack([1.1 * np.cos(1.1 * x) * np.cos(y) + 0.6 * x, -np.sin(1.1 * x) * np.sin(y), o], axis=-1)],
                 axis=-2)
    return np.eye(3) + a * G


def cauchy(F, m):
    """Elastic Cauchy stress of a deformation gradient, 6-vectors."""
    return snp.voigt(snp.elastic_P(F, m) @ np.swapaxes(F, -1, -2) / np.linalg.det(F)[..., None, None])
