"""NumPy restatements shared by tests/test_galerkin_host.py and tests/setup_kernels_worker.py: the meshes, matrices in the
DOF-level layout [node row][d][k][e] as SciPy CSR, the prolongations, and an executor of the vertex-level Galerkin gather's
contribution lists (upper triangle, mirrored) as csrc/solver_kernels.hip pmg_galerkin_kernel runs them."""
import numpy as np
import scipy.sparse as sp

from tests.helpers import load_mesh, tl

MESHES = ["beam_3x2x1", "box", "permuted"]


def mesh(name):
    """beam_3x2x1; the structured 5 x 3 x 3 box; res4 in a seeded random element order"""
    if name == "beam_3x2x1":
        return load_mesh("beam_3x2x1")
    if name == "box":
        return tl.mesh_utils.structured_t10_box(5, 3, 3, 1.0, 0.6, 0.6)
    X, conn = load_mesh("res4")
    return X, np.ascontiguousarray(conn[np.random.default_rng(11).permutation(conn.shape[0])])


def node_adjacency(conn, N):
    """nodes sharing an element: (off, cols), columns ascending"""
    E, k = conn.shape
    inc = sp.csr_matrix((np.ones(k * E), (np.repeat(np.arange(E), k), conn.reshape(-1))), shape=(E, N))
    A = (inc.T @ inc).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32)


def dof_csr(off, cols, vals, n_cols=None):
    """node-block CSR with values in the DOF-level layout [row][d][k][e] -> SciPy CSR (the layout IS that of a sorted
    scalar CSR: row 3 i + d holds [k][e])"""
    n = len(off) - 1
    deg = np.diff(off)
    indptr = np.concatenate([[0], np.cumsum(np.repeat(3 * deg, 3))])
    per_row = [(3 * cols[off[i]:off[i + 1]][:, None] + np.arange(3)[None, :]).reshape(-1) for i in range(n)]
    indices = np.concatenate([np.tile(r, 3) for r in per_row]) if n else np.zeros(0, dtype=np.int64)
    return sp.csr_matrix((np.asarray(vals, dtype=np.float64), indices, indptr), shape=(3 * n, 3 * (n_cols or n)))


def random_symmetric(off, cols, seed):
    """a random symmetric matrix on the node pattern; returns (SciPy CSR, values in the DOF-level layout)"""
    n = len(off) - 1
    rng = np.random.default_rng(seed)
    M = dof_csr(off, cols, rng.normal(size=9 * len(cols)))
    H = (M + M.T).tocsr()
    H.sort_indices()
    assert H.nnz == 9 * len(cols) and H.shape == (3 * n, 3 * n)
    return H, H.data.copy()


def prolongation(par0, par1, Nc):
    """P (3 N x 3 Nc): a fine node is the mean of its parents (a vertex: itself); par < 0: no coarse parent"""
    N = len(par0)
    has = np.where(par0 >= 0)[0]
    Pn = sp.csr_matrix((np.full(2 * len(has), 0.5), (np.concatenate([has, has]), np.concatenate([par0[has], par1[has]]))),
                       shape=(N, Nc))
    return sp.kron(Pn, sp.identity(3), format="csr")


def run_lists(L, Hvals):
    """execute the lists L (dict of the arrays of PmgHost) on H's values: Hc in the DOF-level layout"""
    c_off, nnz_c = L["c_off"], len(L["c_cols"])
    Hc = np.full(9 * nnz_c, np.nan)
    n_upper = len(L["c_upper"])
    t_of = np.repeat(np.arange(n_upper), np.diff(L["con_off"]))
    d, e = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    idx = L["con_base"][:, None, None].astype(np.int64) + d[None] * 3 * L["con_deg"][:, None, None] + e[None]
    blocks = np.zeros((n_upper, 3, 3))
    np.add.at(blocks, t_of, L["con_w"][:, None, None].astype(np.float64) * Hvals[idx])
    deg_c = np.diff(c_off)

    def place(cb):                                                       # address of entry (0, 0) of block cb, row stride
        I = L["cblk_row"][cb]
        return 9 * c_off[I].astype(np.int64) + 3 * (cb - c_off[I]), 3 * deg_c[I]
    cb = L["c_upper"]
    base, stride = place(cb)
    Hc[base[:, None, None] + d[None] * stride[:, None, None] + e[None]] = blocks
    off_diag = L["c_mirror"][cb] != cb
    base, stride = place(L["c_mirror"][cb][off_diag])
    Hc[base[:, None, None] + e[None] * stride[:, None, None] + d[None]] = blocks[off_diag]
    return Hc
