"""NumPy restatement of the field obstacles (DESIGN 3e''): the quadratic B-spline evaluation of a signed-distance grid
with a rigid pose, the per-point force and block with the gap phi in the place of the distance, and the builder (point-
triangle distance by region, sign by the winding number).  A field is a dict: V [nz, ny, nx], origin, spacing, pos, rot,
vel, kappa, mu, eps_v."""
import numpy as np


def field(V, origin, spacing, kappa, mu=0.0, eps_v=1e-3, pos=(0, 0, 0), rot=None, vel=(0, 0, 0)):
    return dict(kind=2, V=np.asarray(V, dtype=float), origin=np.asarray(origin, dtype=float), spacing=float(spacing),
                pos=np.asarray(pos, dtype=float), rot=np.eye(3) if rot is None else np.asarray(rot, dtype=float),
                vel=np.asarray(vel, dtype=float), kappa=float(kappa), mu=float(mu), eps_v=float(eps_v))


def grid_coords(o, x):
    """g = (rot^T (x - pos) - origin) / spacing"""
    return (o["rot"].T @ (np.asarray(x, dtype=float) - o["pos"]) - o["origin"]) / o["spacing"]


def weights(t):
    return (np.array([0.5 * (0.5 - t) ** 2, 0.75 - t * t, 0.5 * (0.5 + t) ** 2]),
            np.array([-(0.5 - t), -2.0 * t, 0.5 + t]))


def evaluate(o, x, force_index=None):
    """(phi, G) at the world point x, or None outside coverage.  force_index: the centre sample (ix, iy, iz) to use in the
    place of the nearest one (the C1 check evaluates a point on a cell face from either side)."""
    V = o["V"]
    n = np.array(V.shape[::-1])
    g = grid_coords(o, x)
    if not np.all((g >= 0.5) & (g <= n - 1.5)):
        return None
    i = np.clip(np.floor(g + 0.5).astype(int), 1, n - 2) if force_index is None else np.asarray(force_index)
    t = g - i
    (wx, dx), (wy, dy), (wz, dz) = weights(t[0]), weights(t[1]), weights(t[2])
    phi, gr = 0.0, np.zeros(3)
    for c in range(3):
        for b in range(3):
            row = V[i[2] - 1 + c, i[1] - 1 + b, i[0] - 1:i[0] + 2]
            rx, rdx = wx @ row, dx @ row
            phi += wz[c] * wy[b] * rx
            gr += np.array([wz[c] * wy[b] * rdx, wz[c] * dy[b] * rx, dz[c] * wy[b] * rx])
    return float(phi), o["rot"] @ (gr / o["spacing"])


def _friction(o, lam0, n0, q, q0, h, f, B):
    u = q - q0 - h * o["vel"]
    u = u - (n0 @ u) * n0
    y, eps = np.linalg.norm(u), o["eps_v"] * h
    if y >= eps:
        f1y, f1p = 1.0 / y, 0.0
    else:
        f1y, f1p = 2 / eps - y / eps ** 2, 2 / eps - 2 * y / eps ** 2
    c0 = o["mu"] * lam0
    f -= c0 * f1y * u
    B += c0 * f1y * (np.eye(3) - np.outer(n0, n0))
    if y > 0:
        B += c0 * (f1p - f1y) / (y * y) * np.outer(u, u)


def force_block(o, w, q, q0, h):
    """(f = -grad Phi, the engine's 3x3 block, in contact) of one point of weight w."""
    f, B, act = np.zeros(3), np.zeros((3, 3)), 0
    e = evaluate(o, q)
    if e is not None and e[0] < 0:
        phi, G = e
        f += o["kappa"] * w * (-phi) * G
        B += o["kappa"] * w * np.outer(G, G)
        act = 1
    if o["mu"] > 0:
        e0 = evaluate(o, q0)
        if e0 is not None and e0[0] < 0:
            gl = np.linalg.norm(e0[1])
            if gl > 0:
                _friction(o, o["kappa"] * w * (-e0[0]) * gl, e0[1] / gl, q, q0, h, f, B)
    return f, B, act


def energy(o, w, q):
    e = evaluate(o, q)
    return 0.0 if e is None else 0.5 * o["kappa"] * w * min(e[0], 0.0) ** 2


def closed_shape_ok(V):
    V = np.asarray(V)
    if V.ndim != 3 or min(V.shape) < 5 or not np.all(np.isfinite(V)):
        return False
    rim = np.ones(V.shape, dtype=bool)
    rim[2:-2, 2:-2, 2:-2] = False
    return bool(np.all(V[rim] > 0))


def sample(f, shape, origin, spacing):
    """V[iz, iy, ix] = f(origin + spacing (ix, iy, iz)); shape = (nx, ny, nz)"""
    nx, ny, nz = shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return f(np.asarray(origin, dtype=float) + spacing * np.stack([ix, iy, iz], axis=-1).astype(float))


# ---- the builder ------------------------------------------------------------------------------------------------------
def point_triangle_dist2(p, a, b, c):
    """Squared distance from p to the triangle (a, b, c): closest point by Voronoi region."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return ap @ ap
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return bp @ bp
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        r = ap - d1 / (d1 - d3) * ab
        return r @ r
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return cp @ cp
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        r = ap - d2 / (d2 - d6) * ac
        return r @ r
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        r = bp - w * (c - b)
        return r @ r
    den = 1.0 / (va + vb + vc)
    r = ap - vb * den * ab - vc * den * ac
    return r @ r


def solid_angle(p, a, b, c):
    a, b, c = a - p, b - p, c - p
    la, lb, lc = np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c)
    return 2.0 * np.arctan2(a @ np.cross(b, c), la * lb * lc + (a @ b) * lc + (b @ c) * la + (c @ a) * lb)


def sdf_point(p, V, T):
    """(signed distance, winding number) of the closed surface (V, T) at p"""
    d2 = min(point_triangle_dist2(p, V[t[0]], V[t[1]], V[t[2]]) for t in T)
    wn = sum(solid_angle(p, V[t[0]], V[t[1]], V[t[2]]) for t in T) / (4 * np.pi)
    d = np.sqrt(d2)
    return (-d if abs(wn) >= 0.5 else d), wn


def _dist2_many(P, a, b, c):
    """point_triangle_dist2 for the points P [n, 3], region by region"""
    ab, ac = b - a, c - a
    ap, bp, cp = P - a, P - b, P - c
    d1, d2, d3, d4, d5, d6 = ap @ ab, ap @ ac, bp @ ab, bp @ ac, cp @ ab, cp @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        den = 1.0 / (va + vb + vc)
        cases = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        cand = [ap, bp, ap - (d1 / (d1 - d3))[:, None] * ab, cp, ap - (d2 / (d2 - d6))[:, None] * ac,
                bp - w_bc[:, None] * (c - b), ap - (vb * den)[:, None] * ab - (vc * den)[:, None] * ac]
    r, done = cand[6].copy(), np.zeros(len(P), dtype=bool)
    for m, v in zip(cases, cand[:6]):
        pick = m & ~done
        r[pick] = v[pick]
        done |= m
    return np.einsum("ij,ij->i", r, r)


def sdf_grid(V, T, shape, origin, spacing):
    """The builder's grid, indexed [iz, iy, ix]: vectorised over the samples, the triangles in ascending order."""
    nx, ny, nz = shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    P = (np.asarray(origin, dtype=float) + spacing * np.stack([ix, iy, iz], axis=-1).astype(float)).reshape(-1, 3)
    d2, omega = np.full(len(P), np.inf), np.zeros(len(P))
    for t in np.asarray(T):
        a, b, c = V[t[0]], V[t[1]], V[t[2]]
        d2 = np.minimum(d2, _dist2_many(P, a, b, c))
        A, B, C = a - P, b - P, c - P
        la, lb, lc = (np.linalg.norm(v, axis=1) for v in (A, B, C))
        det = np.einsum("ij,ij->i", A, np.cross(B, C))
        dot = lambda u, v: np.einsum("ij,ij->i", u, v)                     # noqa: E731
        omega += 2.0 * np.arctan2(det, la * lb * lc + dot(A, B) * lc + dot(B, C) * la + dot(C, A) * lb)
    d = np.sqrt(d2)
    return np.where(np.abs(omega) / (4 * np.pi) >= 0.5, -d, d).reshape(nz, ny, nx)


def check_closed(V, T):
    """The mirror's rule, restated: '' if (V, T) is closed, consistently oriented and without degenerate triangles."""
    V, T = np.asarray(V, dtype=float), np.asarray(T)
    if T.min() < 0 or T.max() >= len(V):
        return "index out of range"
    edges = {}
    for t in T:
        if np.linalg.norm(np.cross(V[t[1]] - V[t[0]], V[t[2]] - V[t[0]])) == 0:
            return "degenerate triangle"
        for k in range(3):
            e = (int(t[k]), int(t[(k + 1) % 3]))
            edges[e] = edges.get(e, 0) + 1
    if any(n != 1 for n in edges.values()):
        return "inconsistent orientation"
    if any((b, a) not in edges for a, b in edges):
        return "open surface"
    return ""


def box_triangles(lo, hi, sub=1):
    """The surface of the box [lo, hi] with every face split into sub x sub cells of two triangles, outward orientation:
    12 sub^2 triangles, shared vertices merged."""
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    verts, index, tris = [], {}, []

    def vid(p):
        key = tuple(np.round((p - lo) / (hi - lo) * sub).astype(int))
        if key not in index:
            index[key] = len(verts)
            verts.append(lo + (hi - lo) * np.array(key) / sub)
        return index[key]

    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        for side in (0, 1):
            for i in range(sub):
                for j in range(sub):
                    def P(a, b):
                        p = np.zeros(3)
                        p[ax] = lo[ax] if side == 0 else hi[ax]
                        p[u] = lo[u] + (hi[u] - lo[u]) * a / sub
                        p[v] = lo[v] + (hi[v] - lo[v]) * b / sub
                        return vid(p)
                    q = [P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1)]
                    if side == 0:
                        q = q[::-1]
                    tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.array(verts), np.array(tris, dtype=np.int32)


def box_distance(p, lo, hi):
    """Analytic signed distance of the box [lo, hi]"""
    c, hw = 0.5 * (np.asarray(lo) + hi), 0.5 * (np.asarray(hi) - lo)
    q = np.abs(np.asarray(p) - c) - hw
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(np.max(q, axis=-1), 0.0)


# ---- mixed lists: analytic obstacles (tests/obstacles_np.py dicts, kind 0 / 1) and fields (kind 2) ---------------------
def point_terms(o, w, q, q0, h):
    """(force, block, gap or None where a field does not cover q, in contact, friction active) of any obstacle kind"""
    from tests import obstacles_np as onp
    if o["kind"] != 2:
        f, B = onp.force_block(o, w, q, q0, h)
        d = onp.distance(o, q)[0]
        return f, B, d, int(d < 0), bool(o["mu"] > 0 and onp.distance(o, q0)[0] < 0)
    f, B, act = force_block(o, w, q, q0, h)
    e, e0 = evaluate(o, q), evaluate(o, q0)
    fric = bool(o["mu"] > 0 and e0 is not None and e0[0] < 0 and np.linalg.norm(e0[1]) > 0)
    return f, B, (None if e is None else e[0]), act, fric


def nodal(obstacles, w, x, xp, h, pinned=()):
    """T10: per-node forces (N, 3), blocks (N, 3, 3) and per obstacle (resultant, nodes in contact)"""
    N = x.shape[0]
    F, B = np.zeros((N, 3)), np.zeros((N, 3, 3))
    res = [[np.zeros(3), 0] for _ in obstacles]
    skip = set(int(i) for i in pinned)
    for i in np.nonzero(w > 0)[0]:
        if int(i) in skip:
            continue
        for k, o in enumerate(obstacles):
            f, b, _, act, _ = point_terms(o, w[i], x[i], xp[i], h)
            F[i] += f
            B[i] += b
            res[k][0] += f
            res[k][1] += act
    return F, B, [(a, c) for a, c in res]


def _idle(o, r, r0):
    """(mask [E, 32] of the points at which obstacle o certainly contributes nothing, the distances of an analytic o):
    vectorised, so that a large mesh does not pay a Python call per point and obstacle.  Analytic: d >= 0 now and (no
    friction or d >= 0 at the start of the step).  Field: neither position is covered; covered points go the long way."""
    if o["kind"] == 2:
        n = np.array(o["V"].shape[::-1])
        out = []
        for q in (r, r0):
            g = ((q - o["pos"]) @ o["rot"] - o["origin"]) / o["spacing"]
            out.append(np.all((g >= 0.5 - 1e-9) & (g <= n - 1.5 + 1e-9), axis=-1))      # a margin: the exact test decides
        return ~(out[0] | out[1]), None
    if o["kind"] == 0:
        d, d0 = (r - o["p"]) @ o["n"], (r0 - o["p"]) @ o["n"]
    else:
        d, d0 = np.linalg.norm(r - o["p"], axis=-1) - o["radius"], np.linalg.norm(r0 - o["p"], axis=-1) - o["radius"]
    tol = 1e-9 * (1.0 + np.abs(d))                                        # near zero the exact test decides
    return (d > tol) & ((o["mu"] <= 0) | (d0 > tol)), d


def ancf_assemble(prob, obstacles, x, xp, h):
    """tests/ancf_obstacles_np.assemble for a mixed list: force [n_coef, 3], hessian_coo (h x the blocks, as triplets), gap (inf where
    nothing covers the point), pressure (a field's term is kappa <-phi> |G|), touched [E], resultants, weights, points."""
    from tests import ancf_obstacles_np as aonp
    kind, dims = prob[0], prob[5]
    ids, Sv, w = aonp.coef_ids(prob), aonp.shape_values(kind, dims), aonp.weights(prob)
    r, r0 = aonp.positions(prob, x), aonp.positions(prob, xp)
    E, n, P = ids.shape[0], np.asarray(x).shape[0], aonp.P
    fp, Cp = np.zeros((E, P, 3)), np.zeros((E, P, 3, 3))
    gap, press = np.full((E, P), np.inf), np.zeros((E, P))
    touched = np.zeros(E, dtype=bool)
    res = [[np.zeros(3), 0] for _ in obstacles]
    idle = [_idle(o, r, r0) for o in obstacles]
    for e in range(E):
        for p in range(P):
            for k, o in enumerate(obstacles):
                if idle[k][0][e, p]:                                 # no force, no block, not in contact, no friction
                    if o["kind"] != 2:
                        gap[e, p] = min(gap[e, p], idle[k][1][e, p])
                    elif evaluate(o, r[e, p]) is not None:
                        gap[e, p] = min(gap[e, p], evaluate(o, r[e, p])[0])
                    continue
                f, b, d, act, fric = point_terms(o, w[e, p], r[e, p], r0[e, p], h)
                fp[e, p] += f
                Cp[e, p] += b
                res[k][0] += f
                res[k][1] += act
                touched[e] |= bool(act) or fric
                if d is not None:
                    gap[e, p] = min(gap[e, p], d)
                    if d < 0:
                        press[e, p] += o["kappa"] * (-d) * (np.linalg.norm(evaluate(o, r[e, p])[1]) if o["kind"] == 2 else 1.0)
    F = np.zeros((n, 3))
    rows, cols, vals = [], [], []                                        # the Hessian (h x the blocks) as triplets
    for e in range(E):
        np.add.at(F, ids[e], Sv.T @ fp[e])
        if touched[e]:
            K = h * np.einsum("pi,pj,pab->iajb", Sv, Sv, Cp[e]).reshape(3 * Sv.shape[1], -1)
            dof = (3 * ids[e][:, None] + np.arange(3)[None, :]).reshape(-1)
            rows.append(np.repeat(dof, dof.size))
            cols.append(np.tile(dof, dof.size))
            vals.append(K.reshape(-1))
    cat = lambda a, t: np.concatenate(a) if a else np.zeros(0, dtype=t)       # noqa: E731
    return dict(force=F, hessian_coo=(cat(rows, np.int64), cat(cols, np.int64), cat(vals, float)), fp=fp, Cp=Cp, gap=gap,
                pressure=press, touched=touched, resultants=[(a, c) for a, c in res], weights=w, points=r)


def coo_on_csr(ro, ci, coo, n):
    """The triplets summed onto the pattern (ro, ci) of an n x n CSR matrix: an array aligned with its values.  Every
    triplet must have a place in the pattern."""
    rows, cols, vals = coo
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro)) * n + np.asarray(ci, dtype=np.int64)
    order = np.argsort(keys)
    pos = np.searchsorted(keys[order], rows * n + cols)
    assert np.all(pos < keys.size) and np.array_equal(keys[order][pos], rows * n + cols)
    out = np.zeros(keys.size)
    np.add.at(out, order[pos], vals)
    return out
