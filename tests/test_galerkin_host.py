"""Host set-up of the vertex-level Galerkin gather (csrc/pmg_host.h) through a small native shim.  H is symmetric, so the
builders keep contribution lists only for the coarse blocks with column >= row (c_upper) and the kernel stores every
off-diagonal block a second time, transposed, at c_mirror.  Checked here without a GPU: the mirror table, the cover, the
lists executed in NumPy against P^T H P, and the refusal of a pattern that lacks a mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import galerkin_np as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-13      # lists against P^T H P, relative to max |Hc|


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("gal") / "libgalerkin_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "galerkin_shim.cc")])
    return C.CDLL(str(so))


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def fetch(shim, N, sizes):
    Nc, nnz_c, n_upper, n_con = (int(v) for v in sizes)
    z = lambda n: np.zeros(n, dtype=np.int32)  # noqa: E731
    L = dict(par0=z(N), par1=z(N), c_off=z(Nc + 1), c_cols=z(nnz_c), cblk_row=z(nnz_c), c_upper=z(n_upper),
             c_mirror=z(nnz_c), con_off=z(n_upper + 1), con_blk=z(n_con), con_base=z(n_con), con_deg=z(n_con),
             con_w=np.zeros(n_con, dtype=np.float32))
    names = ["par0", "par1", "c_off", "c_cols", "cblk_row", "c_upper", "c_mirror", "con_off", "con_blk", "con_base", "con_deg"]
    shim.gal_fetch(*[ip(L[k]) for k in names], L["con_w"].ctypes.data_as(C.POINTER(C.c_float)))
    return L


def check_lists(shim, L, off, cols, seed):
    """everything the issue asks of one set of lists; returns (contributions kept, contributions of the full gather)"""
    Nc, nnz_c = len(L["c_off"]) - 1, len(L["c_cols"])
    ids, mir, row, col = np.arange(nnz_c), L["c_mirror"], L["cblk_row"], L["c_cols"]
    assert np.array_equal(row, np.repeat(np.arange(Nc), np.diff(L["c_off"])))
    # an involution that swaps row and column and fixes exactly the diagonal blocks
    assert np.array_equal(mir[mir], ids)
    assert np.array_equal(row[mir], col) and np.array_equal(col[mir], row)
    assert np.array_equal(mir == ids, row == col)
    # c_upper: the blocks with column >= row, ascending; with their mirrors every block exactly once
    up = L["c_upper"]
    assert np.array_equal(up, ids[col >= row])
    off_diag = up[mir[up] != up]
    assert np.array_equal(np.sort(np.concatenate([up, mir[off_diag]])), ids)
    # lists: one per upper block, none empty, fine blocks ascending (the fixed summation order)
    con_off = L["con_off"]
    assert con_off[0] == 0 and con_off[-1] == len(L["con_w"]) and np.all(np.diff(con_off) >= 1)
    for u in np.where(np.diff(con_off) > 1)[0]:
        assert np.all(np.diff(L["con_blk"][con_off[u]:con_off[u + 1]]) > 0)
    f_row = np.repeat(np.arange(len(off) - 1), np.diff(off))[L["con_blk"]]
    assert np.array_equal(L["con_base"], 9 * off[f_row] + 3 * (L["con_blk"] - off[f_row]))
    assert np.array_equal(L["con_deg"], np.diff(off)[f_row])
    # executed with the mirror store: P^T H P for a random symmetric H on the pattern
    H, Hvals = gn.random_symmetric(off, cols, seed)
    dev = gn.dof_csr(L["c_off"], L["c_cols"], gn.run_lists(L, Hvals))
    assert not np.any(np.isnan(dev.data))                                # every entry of every block was stored
    P = gn.prolongation(L["par0"], L["par1"], Nc)
    ref = (P.T @ H @ P).tocsr()
    err = float(abs(dev - ref).max() / abs(ref).max())
    print(f"lists vs P^T H P: {err:.3e} x max |Hc|; {len(L['con_w'])} contributions for {len(up)} of {nnz_c} blocks")
    assert err <= TOL
    # the lower triangle is the exact transpose of the upper one; a diagonal block is summed in full, entry by entry, so
    # inside it (d, e) and (e, d) are two sums of the same numbers in different orders: equal to rounding
    asym = (dev - dev.T).tocoo()
    off_diag_blocks = asym.row // 3 != asym.col // 3
    assert not np.any(asym.data[off_diag_blocks] != 0.0)
    assert np.all(np.abs(asym.data[~off_diag_blocks]) <= TOL * abs(ref).max())
    # the full gather's size: every (parent of i, parent of j) of every fine block
    npar = np.where(L["par0"] < 0, 0, np.where(L["par0"] == L["par1"], 1, 2))
    full = int(np.sum(npar[np.repeat(np.arange(len(off) - 1), np.diff(off))] * npar[cols]))
    return len(L["con_w"]), full


@pytest.mark.parametrize("name", gn.MESHES)
def test_t10_lists(shim, name):
    X, conn = gn.mesh(name)
    N, E = X.shape[0], conn.shape[0]
    off, cols = gn.node_adjacency(conn, N)
    connT = np.ascontiguousarray(conn.T, dtype=np.int32)                # column-major [10][E]
    sizes = np.zeros(4, dtype=np.int32)
    assert shim.gal_build(N, E, ip(connT), ip(off), ip(cols), ip(sizes)) == 0
    L = fetch(shim, N, sizes)
    kept, full = check_lists(shim, L, off, cols, seed=3)
    n_diag = int(np.diff(L["con_off"])[L["c_cols"][L["c_upper"]] == L["cblk_row"][L["c_upper"]]].sum())
    assert 2 * kept - n_diag == full                                    # exactly the lower triangle's lists are gone
    # a pattern with one mirror removed is refused (an off-diagonal block), one without a diagonal block is not
    lower = int(np.where(L["c_cols"] < L["cblk_row"])[0][0])
    upper = int(np.where(L["c_cols"] > L["cblk_row"])[0][-1])
    diag = int(np.where(L["c_cols"] == L["cblk_row"])[0][0])
    assert shim.gal_mirror_without(-1) == 1
    assert shim.gal_mirror_without(lower) == 0 and shim.gal_mirror_without(upper) == 0
    assert shim.gal_mirror_without(diag) == 1


def ancf_beam_adjacency(n_nodes):
    """coefficient adjacency of a chain of two-node beam elements, four coefficients per node"""
    conn = np.stack([np.concatenate([4 * a + np.arange(4), 4 * (a + 1) + np.arange(4)]) for a in range(n_nodes - 1)])
    return gn.node_adjacency(conn, 4 * n_nodes)


def test_ancf_lists(shim):
    n_nodes = 7
    off, cols = ancf_beam_adjacency(n_nodes)
    sizes = np.zeros(4, dtype=np.int32)
    assert shim.gal_build_ancf(4 * n_nodes, ip(off), ip(cols), ip(sizes)) == 0
    L = fetch(shim, 4 * n_nodes, sizes)
    assert int(sizes[0]) == n_nodes and np.all(np.diff(L["con_off"]) == 1) and np.all(L["con_w"] == 1.0)
    kept, full = check_lists(shim, L, off, cols, seed=5)
    assert kept == len(L["c_upper"]) and full == len(L["c_cols"])
    # a fine pattern without the block (position of node 2, position of node 1): the mirror of (1, 2) is missing
    g = int(np.where((np.repeat(np.arange(4 * n_nodes), np.diff(off)) == 8) & (cols == 4))[0][0])
    off2 = off.copy()
    off2[9:] -= 1
    cols2 = np.ascontiguousarray(np.delete(cols, g))
    assert shim.gal_build_ancf(4 * n_nodes, ip(off2), ip(cols2), ip(sizes)) != 0
