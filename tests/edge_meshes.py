"""T10 meshes at the edges of what the element stage's work lists and launches were written for: one element, element
counts around a multiple of 64, a hub node whose row of H needs more LDS than the default 64 KiB, nodes that belong to
no element, one curved element.  Plain numpy; every builder returns (X [N, 3] float64, conn [E, 10] int32) with the
mid-edge nodes in the order of mesh_utils.EDGES and det J > 0 in every element (tests/test_edge_meshes.py)."""
import importlib

import numpy as np

mu = importlib.import_module("total-lagrangian-fea_amd.mesh_utils")

# counts of every mesh: N nodes, E elements, largest node degree (3x3 blocks in the longest node row of H)
COUNTS = {"one_tet": (10, 1, 10), "star2": (325, 128, 325), "star3": (1285, 512, 1285), "star4": (5125, 2048, 5125),
          "box_192": (405, 192, 65), "box_65": (206, 65, 32), "box_63": (198, 63, 32), "isolated_box": (78, 24, 42),
          "cone_22x20": (2205, 880, 2205)}
# doubles of LDS accumulator the largest row group of the stars needs (9 x the hub's degree), both row-group forms
STAR_ACC_MAX = {"star2": 2925, "star3": 11565, "star4": 46125, "cone_22x20": 19845}


def t10_from_tets(V, tets):
    """(X, conn) of the straight-sided T10 mesh on vertices V [nv, 3] and tets [E, 4] (oriented here): the vertices keep
    their numbers, the mid-edge nodes follow in the order of the sorted unique edges"""
    V = np.asarray(V, dtype=np.float64)
    t = np.array(tets, dtype=np.int64)
    d = V[t[:, 1:]] - V[t[:, :1]]
    flip = np.einsum("ij,ij->i", d[:, 0], np.cross(d[:, 1], d[:, 2])) < 0
    t[flip, 1], t[flip, 2] = t[flip, 2].copy(), t[flip, 1].copy()
    nv = V.shape[0]
    pairs = np.stack([np.sort(t[:, [a, b]], axis=1) for a, b in mu.EDGES], axis=1)      # [E, 6, 2]
    key = pairs[..., 0] * nv + pairs[..., 1]
    used, inv = np.unique(key.ravel(), return_inverse=True)
    mids = 0.5 * (V[used // nv] + V[used % nv])
    conn = np.concatenate([t, nv + inv.reshape(-1, 6)], axis=1).astype(np.int32)
    return np.vstack([V, mids]), np.ascontiguousarray(conn)


def one_tet():
    return t10_from_tets([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.2, 0.9, 0.0], [0.1, 0.3, 0.8]], [[0, 1, 2, 3]])


def star(nsub):
    """The 8 x 4^nsub surface triangles of an octahedron subdivided nsub times (vertices on the unit sphere), each coned
    to the centre: the hub is the last vertex before the mid-edge nodes and belongs to every element, so its row of H
    has one block per node of the mesh."""
    verts = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    tris = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(nsub):
        mid, new = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = 0.5 * (np.asarray(verts[a]) + np.asarray(verts[b]))
                verts.append(tuple(p / np.linalg.norm(p)))
                mid[k] = len(verts) - 1
            return mid[k]

        for a, b, c in tris:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            new += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        tris = new
    hub = len(verts)
    V = np.vstack([np.asarray(verts, dtype=np.float64), np.zeros((1, 3))])
    return t10_from_tets(V, [(a, b, c, hub) for a, b, c in tris])


def cone(n, m):
    """A sphere of m latitude rings of n points and two poles (2 n m triangles), coned to the centre like star(): the hub's
    degree is 5 n m + 5.  cone(22, 20): 2 205 blocks, a row of 155 KiB -- it fits assemble_rows_kernel within the 160 KiB
    a workgroup of the MI355X can have, and neither fused form, whose staging comes on top."""
    th = np.pi * (np.arange(m) + 1) / (m + 1)
    ph = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n))], axis=2)
    V = np.vstack([ring.reshape(-1, 3), [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0]]])
    top, bottom, hub = n * m, n * m + 1, n * m + 2
    tris = []
    for j in range(n):
        k = (j + 1) % n
        tris += [(top, j, k), (bottom, (m - 1) * n + k, (m - 1) * n + j)]
        for r in range(m - 1):
            a, b, c, d = r * n + j, r * n + k, (r + 1) * n + j, (r + 1) * n + k
            tris += [(a, c, d), (a, d, b)]
    return t10_from_tets(V, [(a, b, c, hub) for a, b, c in tris])


def star_hub(X, conn):
    """the node that belongs to every element"""
    hub = set(conn[0].tolist())
    for row in conn[1:]:
        hub &= set(row.tolist())
    assert len(hub) == 1
    return hub.pop()


def compact(X, conn):
    """drops the nodes no element uses and renumbers the rest in their old order"""
    used = np.unique(conn)
    new = -np.ones(X.shape[0], dtype=np.int64)
    new[used] = np.arange(len(used))
    return X[used].copy(), np.ascontiguousarray(new[conn], dtype=np.int32)


def box_192():
    return mu.structured_t10_box(4, 4, 2)


def box_minus(n_drop):
    """structured_t10_box(1, 1, 11) (66 elements) without its last n_drop elements; no node is left without an element"""
    X, conn = mu.structured_t10_box(1, 1, 11)
    return compact(X, conn[:conn.shape[0] - n_drop])


def box_65():
    return box_minus(1)


def box_63():
    return box_minus(3)


# positions of the three unused nodes of with_isolated: the first lies in the plane x = 0 (tests.helpers.fixed_x0 pins it),
# the last outside the body's bounding box; none coincides with a lattice node
ISOLATED_AT = np.array([[0.0, 0.37, 0.41], [0.6, 0.3, 0.7], [1.3, 0.2, 0.1]])


def with_isolated(X, conn):
    """(X', conn', isolated): three nodes that belong to no element inserted as node 0, as node N // 2 and as the last
    node; the connectivity is shifted accordingly"""
    N = X.shape[0]
    at = [0, N // 2, N + 2]                                   # final indices of the new nodes
    keep = np.setdiff1d(np.arange(N + 3), at)                 # final index of old node i
    Xn = np.zeros((N + 3, 3))
    Xn[keep] = X
    Xn[at] = ISOLATED_AT
    return Xn, np.ascontiguousarray(keep[conn], dtype=np.int32), np.array(at, dtype=np.int32)


def isolated_box():
    X, conn = mu.structured_t10_box(2, 2, 1)
    return with_isolated(X, conn)


def curved(X, conn):
    """one mid-edge node of element 0 off its edge, as in tests/test_gpu_parity.py::test_hessian_affine_and_general_forms:
    the mesh is no longer straight-sided and takes the general form of the fused assembly"""
    Xc = X.copy()
    edge = np.linalg.norm(X[conn[0, 0]] - X[conn[0, 1]])
    Xc[int(conn[0, 4])] += 0.03 * edge * np.array([0.3, -0.5, 0.8])
    return Xc, conn


def build(name):
    """(X, conn) by name: the names of COUNTS, 'curved_star2' / 'curved_star3'"""
    if name.startswith("curved_"):
        return curved(*build(name[len("curved_"):]))
    if name.startswith("star"):
        return star(int(name[4:]))
    if name.startswith("cone_"):
        return cone(*(int(v) for v in name[5:].split("x")))
    if name == "isolated_box":
        return isolated_box()[:2]
    return {"one_tet": one_tet, "box_192": box_192, "box_65": box_65, "box_63": box_63}[name]()
