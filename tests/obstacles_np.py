"""NumPy restatement of the rigid-obstacle model: surface weights, the per-node energy, force and 3x3
Hessian block of half-spaces and spheres, and regularised friction with the start-of-step normal force."""
import numpy as np

FACES = ((0, 1, 2, 4, 5, 6), (0, 1, 3, 4, 8, 7), (0, 2, 3, 6, 9, 7), (1, 2, 3, 5, 9, 8))  # T10 faces: corners, mid-edges


def surface_weights(X, conn):
    """w_i = sum of A_f / 6 over the boundary faces (one tet only) incident to node i; A_f the corner-triangle area."""
    seen = {}
    for e, c in enumerate(np.asarray(conn)):
        for f in FACES:
            seen.setdefault(tuple(sorted(int(c[t]) for t in f[:3])), []).append([int(c[t]) for t in f])
    w = np.zeros(X.shape[0])
    for lst in seen.values():
        if len(lst) == 1:
            nd = lst[0]
            A = 0.5 * np.linalg.norm(np.cross(X[nd[1]] - X[nd[0]], X[nd[2]] - X[nd[0]]))
            w[nd] += A / 6.0
    return w


def distance(o, q):
    """Signed distance and outward unit normal of obstacle o (dict: kind 0 plane p, n | kind 1 sphere p, radius)."""
    if o["kind"] == 0:
        n = np.asarray(o["n"], dtype=float)
        return float(n @ (q - o["p"])), n
    r = q - np.asarray(o["p"], dtype=float)
    rl = np.linalg.norm(r)
    n = r / rl if rl > 0 else np.array([0.0, 0.0, 1.0])
    return float(rl - o["radius"]), n


def _f0(y, eps):
    return y * y / eps - y ** 3 / (3 * eps * eps) + eps / 3 if y < eps else y


def energy(o, w, q, q0, h):
    """Phi of one node: normal penalty plus friction (lam0, P_t from the start-of-step position q0)."""
    d, _ = distance(o, q)
    phi = 0.5 * o["kappa"] * w * min(d, 0.0) ** 2
    if o["mu"] > 0:
        d0, n0 = distance(o, q0)
        if d0 < 0:
            u = q - q0 - h * np.asarray(o["vel"], dtype=float)
            u = u - (n0 @ u) * n0
            phi += o["mu"] * o["kappa"] * w * (-d0) * _f0(np.linalg.norm(u), o["eps_v"] * h)
    return phi


def force_block(o, w, q, q0, h):
    """(f = -grad Phi, the engine's 3x3 block): exact for a half-space, Gauss-Newton normal term for a sphere."""
    f, B = np.zeros(3), np.zeros((3, 3))
    d, n = distance(o, q)
    if d < 0:
        f += o["kappa"] * w * (-d) * n
        B += o["kappa"] * w * np.outer(n, n)
    if o["mu"] > 0:
        d0, n0 = distance(o, q0)
        if d0 < 0:
            lam0 = o["kappa"] * w * (-d0)
            u = q - q0 - h * np.asarray(o["vel"], dtype=float)
            u = u - (n0 @ u) * n0
            y, eps = np.linalg.norm(u), o["eps_v"] * h
            if y >= eps:
                f1y, f1p = 1.0 / y, 0.0
            else:
                f1y, f1p = 2 / eps - y / eps ** 2, 2 / eps - 2 * y / eps ** 2
            c0 = o["mu"] * lam0
            f -= c0 * f1y * u
            Pt = np.eye(3) - np.outer(n0, n0)
            B += c0 * f1y * Pt
            if y > 0:
                B += c0 * (f1p - f1y) / (y * y) * np.outer(u, u)
    return f, B


def nodal(obstacles, w, x, xp, h, pinned=()):
    """Per-node forces (N, 3) and blocks (N, 3, 3) of a list of obstacles; pinned nodes take no part."""
    N = x.shape[0]
    F, B = np.zeros((N, 3)), np.zeros((N, 3, 3))
    skip = set(int(i) for i in pinned)
    for i in np.nonzero(w > 0)[0]:
        if int(i) in skip:
            continue
        for o in obstacles:
            f, b = force_block(o, w[i], x[i], xp[i], h)
            F[i] += f
            B[i] += b
    return F, B
