"""ANCF-3243 beam and ANCF-3443 shell meshes at the edges of what the two-kernel element stage was written for: one
element, five elements (one live wave and three shadows in the last workgroup of TLFEA_TANGENT_WPB=4), a hub node whose
row of H has one block per coefficient of the mesh (up to more than 64 KiB of LDS in assemble_rows_kernel, a whole number
of its 8-element chunks or one element more), per-element dimensions that differ, mesh nodes of no element.  Plain numpy.

Every builder returns (kind, x12, y12, z12, conn_nodes, L, W, H): the coefficient arrays of 4 n_nodes entries (r, r_x, r_y,
r_z per node), the node connectivity [E, 2] / [E, 4] int32 and the dimensions per element.  The meshes need not be physical
(the shells of a fan overlap); det J > 0 at every force and mass point is checked in tests/test_ancf_edge_meshes.py."""
import numpy as np

BEAM_DIMS = (0.5, 0.1, 0.1)        # L, W, H of every beam
SHELL_DIMS = (0.5, 0.4, 0.05)      # ... of every shell
CAP_HALF_ANGLE = 0.6               # fan3243: the tips lie within this angle of +x, seen from the hub
GOLDEN_ANGLE = np.pi * (3.0 - np.sqrt(5.0))


def coefficients(pos):
    """(x12, y12, z12) of nodes at pos [n, 3] that all carry the gradients r_x = e_x, r_y = e_y, r_z = e_z"""
    pos = np.asarray(pos, dtype=np.float64)
    c = np.zeros((pos.shape[0], 4, 3))
    c[:, 0, :] = pos
    c[:, 1:, :] = np.eye(3)[None, :, :]
    c = c.reshape(-1, 3)
    return tuple(np.ascontiguousarray(c[:, k]) for k in range(3))


def mesh(kind, pos, conn):
    conn = np.ascontiguousarray(conn, dtype=np.int32)
    dims = BEAM_DIMS if kind == 3243 else SHELL_DIMS
    return (kind,) + coefficients(pos) + (conn,) + tuple(np.full(conn.shape[0], v) for v in dims)


def chain(n):
    """n beams in a row along x; beam e joins nodes e and e + 1"""
    L = BEAM_DIMS[0]
    pos = np.zeros((n + 1, 3))
    pos[:, 0] = L * np.arange(n + 1)
    return mesh(3243, pos, np.stack([np.arange(n), np.arange(n) + 1], axis=1))


def strip(n):
    """n shells in a row along x; node 2 i is the lower and 2 i + 1 the upper node of column i, the corners of shell e
    run counter-clockwise from its lower left one"""
    L, W, _ = SHELL_DIMS
    pos = np.zeros((2 * (n + 1), 3))
    pos[0::2, 0] = pos[1::2, 0] = L * np.arange(n + 1)
    pos[1::2, 1] = W
    e = np.arange(n)
    return mesh(3443, pos, np.stack([2 * e, 2 * e + 2, 2 * e + 3, 2 * e + 1], axis=1))


def one_beam():
    return chain(1)


def one_shell():
    return strip(1)


def chain5():
    return chain(5)


def strip5():
    return strip(5)


def fan3243(k):
    """k beams from the hub (node 0, at the origin) to k tips at distance L on a spherical cap of half-angle 0.6 rad about
    +x (a spiral: equal steps in the cosine, the golden angle in azimuth).  Beam e joins the hub and node e + 1; the hub's
    row of H has 4 + 4 k blocks."""
    L = BEAM_DIMS[0]
    i = np.arange(k)
    ct = 1.0 - (1.0 - np.cos(CAP_HALF_ANGLE)) * (i + 0.5) / k
    st, ph = np.sqrt(1.0 - ct * ct), GOLDEN_ANGLE * i
    tips = L * np.stack([ct, st * np.cos(ph), st * np.sin(ph)], axis=1)
    return mesh(3243, np.vstack([np.zeros((1, 3)), tips]), np.stack([np.zeros(k, dtype=np.int64), i + 1], axis=1))


def fan3443(k):
    """k shells that share their first corner, the hub (node 0, at the origin); shell e owns nodes 3 e + 1 .. 3 e + 3, its
    other corners: those of the L x W rectangle rotated about z by an angle within +-0.3 rad and lifted in z by up to
    +-0.1.  The hub's row of H has 4 + 12 k blocks."""
    L, W, _ = SHELL_DIMS
    e = np.arange(k)
    ang, dz = 0.3 * np.cos(GOLDEN_ANGLE * e), 0.1 * np.sin(1.3 * e + 0.5)
    corners = np.array([[L, 0.0], [L, W], [0.0, W]])                       # P2, P3, P4 of the unrotated shell
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    own = np.stack([c * corners[None, :, 0] - s * corners[None, :, 1], s * corners[None, :, 0] + c * corners[None, :, 1],
                    np.broadcast_to(dz[:, None], (k, 3))], axis=2)          # [k, 3 corners, xyz]
    conn = np.concatenate([np.zeros((k, 1), dtype=np.int64), 3 * e[:, None] + 1 + np.arange(3)[None, :]], axis=1)
    return mesh(3443, np.vstack([np.zeros((1, 3)), own.reshape(-1, 3)]), conn)


def graded(m):
    """the dimensions of element e scaled by 1 + 0.2 sin(e), the coefficients left where they are: B^-1 and det J differ
    from element to element"""
    kind, x, y, z, conn, L, W, H = m
    f = 1.0 + 0.2 * np.sin(np.arange(conn.shape[0]))
    return kind, x, y, z, conn, L * f, W * f, H * f


ISOLATED_AT = np.array([[-0.3, 0.7, 0.2], [0.9, -0.6, 0.4]])     # away from every node of chain5 and strip5


def with_isolated(m):
    """two mesh nodes (eight coefficients) appended that belong to no element; the configurations pin the first of them"""
    kind, x, y, z, conn, L, W, H = m
    xi, yi, zi = coefficients(ISOLATED_AT)
    return kind, np.concatenate([x, xi]), np.concatenate([y, yi]), np.concatenate([z, zi]), conn, L, W, H


def unused_nodes(m):
    """mesh nodes of no element, ascending"""
    return np.setdiff1d(np.arange(len(m[1]) // 4), m[4]).astype(np.int32)


def node_coefficients(nodes):
    """the four coefficient indices of every node, ascending per node"""
    return (4 * np.atleast_1d(np.asarray(nodes, dtype=np.int64))[:, None] + np.arange(4)[None, :]).reshape(-1).astype(np.int32)


def hub_row_blocks(m):
    """3 x 3 blocks in the longest coefficient row of H: the coefficients of every node that shares an element with the
    best connected node"""
    conn = m[4]
    best = 0
    for n in np.unique(conn):
        best = max(best, len(np.unique(conn[np.any(conn == n, axis=1)])))
    return 4 * best


def assemble_rows_lds_bytes(m):
    """dynamic LDS of assemble_rows_kernel for this mesh: 9 doubles per block of the longest row"""
    return 9 * 8 * hub_row_blocks(m)


BASE = {"one_beam": one_beam, "one_shell": one_shell, "chain5": chain5, "strip5": strip5}
# coefficients N, elements E, blocks in the longest row
COUNTS = {"one_beam": (8, 1, 8), "one_shell": (16, 1, 16), "chain5": (24, 5, 12), "strip5": (48, 5, 24),
          "fan3243_8": (36, 8, 36), "fan3243_9": (40, 9, 40), "fan3243_230": (924, 230, 924),
          "fan3443_8": (100, 8, 100), "fan3443_9": (112, 9, 112), "fan3443_80": (964, 80, 964),
          "graded_chain5": (24, 5, 12), "graded_strip5": (48, 5, 24),
          "isolated_chain5": (32, 5, 12), "isolated_strip5": (56, 5, 24)}


def build(name):
    """a mesh by name: the names of COUNTS"""
    if name.startswith("graded_"):
        return graded(build(name[len("graded_"):]))
    if name.startswith("isolated_"):
        return with_isolated(build(name[len("isolated_"):]))
    if name.startswith("fan3243_"):
        return fan3243(int(name[8:]))
    if name.startswith("fan3443_"):
        return fan3443(int(name[8:]))
    return BASE[name]()
