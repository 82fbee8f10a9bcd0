"""NumPy restatement of the surface loads on the boundary faces of a T10 mesh (DESIGN 3h'): the boundary faces in
ascending (element, local face) order with their six nodes ordered outward, the dead traction on the reference face and
the follower pressure on the current one, both on the 6-point degree-4 triangle rule; and the current volume of the mesh,
whose derivative the pressure is."""
import numpy as np

from tests.obstacles_np import FACES

EDGES = ((0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3))      # mid-edge nodes 4..9 of the tet


def rule6():
    """(xi, eta, w): the 6-point rule of degree 4 on the unit triangle (weights sum to 1/2), in closed form"""
    s10 = np.sqrt(10.0)
    r = np.sqrt(38.0 - 44.0 * np.sqrt(0.4))
    w = np.sqrt(213125.0 - 53320.0 * s10)
    pts = []
    for a, wa in (((8.0 - s10 + r) / 18.0, (620.0 + w) / 3720.0), ((8.0 - s10 - r) / 18.0, (620.0 - w) / 3720.0)):
        pts += [(a, a, 0.5 * wa), (1.0 - 2.0 * a, a, 0.5 * wa), (a, 1.0 - 2.0 * a, 0.5 * wa)]
    return np.array(pts)


def rule3():
    """the 3-point rule of degree 2"""
    return np.array([(1 / 6, 1 / 6, 1 / 6), (2 / 3, 1 / 6, 1 / 6), (1 / 6, 2 / 3, 1 / 6)])


def rule_duffy(n):
    """n x n Gauss points collapsed onto the triangle: exact to degree 2 n - 2"""
    g, w = np.polynomial.legendre.leggauss(n)
    u, wu = 0.5 * (g + 1.0), 0.5 * w
    return np.array([(u[i], u[j] * (1.0 - u[i]), wu[i] * wu[j] * (1.0 - u[i])) for i in range(n) for j in range(n)])


def tri6(xi, eta):
    """(N [6], dN/dxi [6], dN/deta [6]) of the quadratic triangle: corners 0 1 2, mid-edge nodes 01 12 02"""
    l0 = 1.0 - xi - eta
    N = np.array([l0 * (2 * l0 - 1), xi * (2 * xi - 1), eta * (2 * eta - 1), 4 * l0 * xi, 4 * xi * eta, 4 * l0 * eta])
    dx = np.array([-(4 * l0 - 1), 4 * xi - 1, 0.0, 4 * (l0 - xi), 4 * eta, -4 * eta])
    de = np.array([-(4 * l0 - 1), 0.0, 4 * eta - 1, -4 * xi, 4 * xi, 4 * (l0 - eta)])
    return N, dx, de


def boundary_faces(X, conn):
    """(elem [F], local_face [F], nodes [F, 6]): the faces that belong to one tet only, ascending (element, local face);
    nodes reordered (two corners and their mid-edge nodes swapped) so that X_xi x X_eta points away from the tet's fourth
    vertex"""
    conn = np.asarray(conn)
    count = {}
    for c in conn:
        for f in FACES:
            key = tuple(sorted(int(c[t]) for t in f[:3]))
            count[key] = count.get(key, 0) + 1
    elem, lf, nodes = [], [], []
    for e, c in enumerate(conn):
        for k, f in enumerate(FACES):
            if count[tuple(sorted(int(c[t]) for t in f[:3]))] != 1:
                continue
            nd = [int(c[t]) for t in f]
            fourth = int(c[6 - f[0] - f[1] - f[2]])
            n = np.cross(X[nd[1]] - X[nd[0]], X[nd[2]] - X[nd[0]])
            if n @ (X[fourth] - X[nd[0]]) > 0:
                nd = [nd[0], nd[2], nd[1], nd[5], nd[4], nd[3]]
            elem.append(e)
            lf.append(k)
            nodes.append(nd)
    return np.array(elem, dtype=np.int32), np.array(lf, dtype=np.int32), np.array(nodes, dtype=np.int32).reshape(-1, 6)


def face_geometry(X, nodes):
    """(centroid [F, 3], outward unit normal [F, 3], area [F]) of the corner triangles in the reference configuration"""
    a, b, c = X[nodes[:, 0]], X[nodes[:, 1]], X[nodes[:, 2]]
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1)
    return (a + b + c) / 3.0, n / ln[:, None], 0.5 * ln


def traction_rows(X, nd, t, rule=None):
    """[6, 3]: f_a = t sum_q w_q N_a(q) |X_xi x X_eta|(q) on one face"""
    rule = rule6() if rule is None else rule
    w = np.zeros(6)
    for xi, eta, wq in rule:
        N, dx, de = tri6(xi, eta)
        w += wq * N * np.linalg.norm(np.cross(dx @ X[nd], de @ X[nd]))
    return np.outer(w, np.asarray(t, dtype=float))


def pressure_rows(x, nd, p, rule=None):
    """[6, 3]: f_a = -p sum_q w_q N_a(q) (r_xi x r_eta)(q) on one face at the positions x"""
    rule = rule6() if rule is None else rule
    f = np.zeros((6, 3))
    for xi, eta, wq in rule:
        N, dx, de = tri6(xi, eta)
        f += np.outer(N, -p * wq * np.cross(dx @ x[nd], de @ x[nd]))
    return f


def traction_force(X, nodes, faces, t, rule=None):
    F = np.zeros_like(X)
    for k in faces:
        np.add.at(F, nodes[k], traction_rows(X, nodes[k], t, rule))
    return F


def pressure_force(x, nodes, faces, p, rule=None):
    F = np.zeros_like(x)
    for k in faces:
        np.add.at(F, nodes[k], pressure_rows(x, nodes[k], p, rule))
    return F


def total(X, x, nodes, loads=(), gravity_force=None):
    """[N, 3] load of a list of dicts(kind 0 | 1, faces, value, scale) on the boundary faces `nodes`, plus a given
    gravity vector; several pressures on one face add into one effective pressure first, as the host does"""
    F = np.zeros_like(X) if gravity_force is None else np.array(gravity_force, dtype=float).reshape(-1, 3)
    pe = np.zeros(len(nodes))
    for ld in loads:
        if ld["kind"] == 0:
            F = F + ld["scale"] * traction_force(X, nodes, ld["faces"], ld["value"])
        else:
            pe[np.asarray(ld["faces"], dtype=int)] += ld["scale"] * ld["value"]
    for k in np.nonzero(pe)[0]:
        np.add.at(F, nodes[k], pressure_rows(x, nodes[k], pe[k]))
    return F


def volume(x, conn, rule):
    """sum of the current element volumes: det(dx / d(L1, L2, L3)) is cubic, so a degree-3 rule (qx, qy, qz, qw) is exact"""
    qx, qy, qz, qw = rule
    V = 0.0
    for L1, L2, L3, w in zip(qx, qy, qz, qw):
        L = np.array([1.0 - L1 - L2 - L3, L1, L2, L3])
        dL = np.array([[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        dN = np.zeros((10, 3))
        for i in range(4):
            dN[i] = (4 * L[i] - 1) * dL[i]
        for m, (i, j) in enumerate(EDGES):
            dN[4 + m] = 4 * (L[i] * dL[j] + L[j] * dL[i])
        J = np.einsum("ad,eac->ecd", dN, x[np.asarray(conn)])
        V += w * np.linalg.det(J).sum()
    return V
