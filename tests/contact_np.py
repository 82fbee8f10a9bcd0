"""NumPy restatement of the hydroelastic contact rules (broadphase filters, narrowphase patch, patch forces), written
from the rules themselves: the yardstick of the GPU contact kernels in tests/test_contact.py and
tests/test_gpu_contact.py.  Loops are per pair; meant for meshes of a few hundred elements."""
import numpy as np

AREA_EPS = 1e-18
NORMAL_EPS = 1e-9
V_REG = 1e-3


def element_boxes(X, conn):
    P = X[conn]                       # E x npe x 3
    return P.min(axis=1), P.max(axis=1)


def brute_force_pairs(X, conn, mesh_ids, self_collision):
    """All (i < j) with overlapping closed boxes, other meshes only -- or, with self collision, also same-mesh pairs
    that share no node; sorted by (i, j)."""
    lo, hi = element_boxes(X, conn)
    E = conn.shape[0]
    mesh_ids = np.zeros(E, dtype=int) if mesh_ids is None else np.asarray(mesh_ids)
    ov = np.all((lo[:, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[:, None, :]), axis=2)
    ii, jj = np.nonzero(np.triu(ov, 1))
    keep = []
    for i, j in zip(ii, jj):
        if mesh_ids[i] == mesh_ids[j]:
            if not self_collision or np.intersect1d(conn[i], conn[j]).size:
                continue
        keep.append((i, j))
    return np.array(keep, dtype=np.int64).reshape(-1, 2)


def affine_fit(v, p):
    """p(x) = a.x + b through 4 corners; None for a degenerate tet."""
    e1, e2, e3 = v[1] - v[0], v[2] - v[0], v[3] - v[0]
    c23, c31, c12 = np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)
    det = e1 @ c23
    if not abs(det) > 1e-14 * np.linalg.norm(e1) * np.linalg.norm(e2) * np.linalg.norm(e3):
        return None
    a = ((p[1] - p[0]) * c23 + (p[2] - p[0]) * c31 + (p[3] - p[0]) * c12) / det
    return a, p[0] - a @ v[0]


def barycentric(v, x):
    e1, e2, e3, r = v[1] - v[0], v[2] - v[0], v[3] - v[0], x - v[0]
    det = e1 @ np.cross(e2, e3)
    w1, w2, w3 = r @ np.cross(e2, e3) / det, e1 @ np.cross(r, e3) / det, e1 @ np.cross(e2, r) / det
    return np.array([1.0 - w1 - w2 - w3, w1, w2, w3])


def _edge(a, b, da, db):
    return a + (da / (da - db)) * (b - a)


def plane_tet(v, n, c):
    """Plane n.x + c = 0 cut with a tet, in cyclic order (vertices with n.x + c >= 0 count as the positive side)."""
    d = v @ n + c
    pos = [k for k in range(4) if d[k] >= 0.0]
    neg = [k for k in range(4) if d[k] < 0.0]
    if not pos or not neg:
        return []
    if len(pos) == 2:
        a, b = pos
        p, q = neg
        return [_edge(v[a], v[p], d[a], d[p]), _edge(v[a], v[q], d[a], d[q]),
                _edge(v[b], v[q], d[b], d[q]), _edge(v[b], v[p], d[b], d[p])]
    one, three = (pos, neg) if len(pos) == 1 else (neg, pos)
    return [_edge(v[one[0]], v[t], d[one[0]], d[t]) for t in three]


def clip_tet(poly, v):
    """Sutherland-Hodgman against the 4 half-spaces of a tet (faces in the order opposite vertex 0..3)."""
    for f in range(4):
        if not poly:
            break
        q0, q1, q2 = v[(f + 1) % 4], v[(f + 2) % 4], v[(f + 3) % 4]
        nf = np.cross(q1 - q0, q2 - q0)
        if nf @ (v[f] - q0) < 0.0:
            nf = -nf
        out = []
        for k in range(len(poly)):
            P, Q = poly[k], poly[(k + 1) % len(poly)]
            sp, sq = nf @ (P - q0), nf @ (Q - q0)
            if sp >= 0.0 and len(out) < 8:
                out.append(P)
            if (sp >= 0.0) != (sq >= 0.0) and len(out) < 8:
                out.append(_edge(P, Q, sp, sq))
        poly = out
    return poly


def area_centroid(poly):
    p0 = poly[0]
    cr = [np.cross(poly[i] - p0, poly[i + 1] - p0) for i in range(1, len(poly) - 1)]
    s = np.sum(cr, axis=0)
    sn = np.linalg.norm(s)
    area = 0.5 * sn
    if not area >= AREA_EPS:
        return area, None
    u = s / sn
    w = np.array([c @ u for c in cr])
    tri = np.array([p0 + poly[i] + poly[i + 1] for i in range(1, len(poly) - 1)])
    return area, (w @ tri) / (3.0 * w.sum())


def patch(vA, pA, vB, pB, tetA=-1, tetB=-1):
    """One pair; tet A must be on the mesh with the lower id.  -> dict of the ContactPatch fields."""
    out = dict(vertices=np.zeros((0, 3)), normal=np.zeros(3), centroid=np.zeros(3), area=0.0, g_A=0.0, g_B=0.0,
               p_equilibrium=0.0, tetA=tetA, tetB=tetB, isValid=False, validOrientation=False)
    fa, fb = affine_fit(vA, pA), affine_fit(vB, pB)
    if fa is None or fb is None:
        return out
    (aA, bA), (aB, bB) = fa, fb
    n, c = aA - aB, bA - bB
    nn = np.linalg.norm(n)
    if nn < NORMAL_EPS:
        return out
    poly = plane_tet(vA, n, c)
    if len(poly) >= 3:
        poly = clip_tet(poly, vB)
    if len(poly) < 3:
        return out
    area, cen = area_centroid(poly)
    if cen is None:
        return out
    nhat = n / nn
    gA, gB = -(aA @ nhat), aB @ nhat
    orient = True
    if gA <= 0 or gB <= 0:
        nhat, gA, gB = -nhat, -gA, -gB
        if gA <= 0 or gB <= 0:
            nhat, gA, gB, orient = -nhat, -gA, -gB, False
    out.update(vertices=np.array(poly), normal=nhat, centroid=cen, area=area, g_A=gA, g_B=gB,
               p_equilibrium=aA @ cen + bA, isValid=True, validOrientation=orient)
    return out


def patch_force(pt, vA, vB, velA=None, velB=None, damping=0.0, friction=0.0):
    """-> (F on tet B, barycentric weights in A, in B); F is None when the patch applies nothing."""
    if not (pt["isValid"] and pt["validOrientation"] and pt["area"] > AREA_EPS):
        return None, None, None
    n, cen, A = pt["normal"], pt["centroid"], pt["area"]
    wA, wB = barycentric(vA, cen), barycentric(vB, cen)
    p = pt["p_equilibrium"]
    rel = velA is not None and (damping > 0.0 or friction > 0.0)
    if rel:
        vr = wB @ velB - wA @ velA
        vn = vr @ n
        if damping > 0.0:
            p = p * max(0.0, 1.0 - damping * vn)
    F = p * A * n
    if rel and friction > 0.0:
        vt = vr - vn * n
        st = np.linalg.norm(vt)
        if st > 0.0:
            F = F - friction * abs(p * A) * st / (st + V_REG) * (vt / st)
    return F, wA, wB


def contact(X, conn, pressure, mesh_ids, pairs, vel=None, damping=0.0, friction=0.0):
    """Patches of `pairs` and the 3N interleaved nodal contact force (the GPU's rules, summed in any order)."""
    mesh_ids = np.zeros(conn.shape[0], dtype=int) if mesh_ids is None else np.asarray(mesh_ids)
    V = None if vel is None else np.asarray(vel).reshape(-1, 3)
    f = np.zeros((X.shape[0], 3))
    patches = []
    for i, j in pairs:
        a, b = (j, i) if mesh_ids[i] > mesh_ids[j] else (i, j)
        ca, cb = conn[a, :4], conn[b, :4]
        pt = patch(X[ca], pressure[ca], X[cb], pressure[cb], a, b)
        patches.append(pt)
        F, wA, wB = patch_force(pt, X[ca], X[cb], None if V is None else V[ca], None if V is None else V[cb],
                                damping, friction)
        if F is None:
            continue
        np.add.at(f, ca, -wA[:, None] * F[None, :])
        np.add.at(f, cb, wB[:, None] * F[None, :])
    return patches, f.reshape(-1)
