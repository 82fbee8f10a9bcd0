"""Host lists of the streamed build of the restricted fine operator (csrc/pmg_host.h: con_pos, pos_off,
pmg_rop_long_rows) through a small native shim, without a GPU.  The build kernel takes the children of a coarse row in
ascending order, reads each child's row of H front to back and adds block k into the element con_pos gives of an image of
the R row.  Checked on the meshes of tests/setup_kernels_worker.py:

  * every con_pos entry is searchsorted(columns of the R row, column of the fine block), the layout is [row][child][k] with
    one prefix entry per child, and no position repeats within one child;
  * the lists executed in NumPy as the kernel executes them reproduce P^T H of the oracle's H to 1e-15 x max |P^T H|
    (weights 1 and 1/2 are exact and a block sums at most a handful of terms: only the order of a sum of two to six
    doubles separates the two evaluations, and most entries have one or two terms);
  * the long-row list is exactly the rows beyond the capacity, ascending, for capacities 4, 16 and 128."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import galerkin_np as gn
from tests.helpers import MATERIALS, fixed_x0, make_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ["beam_3x2x1", "box", "permuted"]
_lists = {}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("rops") / "librop_stream_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "rop_stream_shim.cc")])
    return C.CDLL(str(so))


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def lists(shim, name):
    """the shim holds one build at a time: build, copy everything out (the long-row lists too), keep it"""
    if name in _lists:
        return _lists[name]
    X, conn = gn.mesh(name)
    N, E = X.shape[0], conn.shape[0]
    off, cols = gn.node_adjacency(conn, N)
    off, cols = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    connT = np.ascontiguousarray(conn.T, dtype=np.int32)                # column-major [10][E]
    sizes = np.zeros(4, dtype=np.int32)
    assert shim.rops_build(N, E, ip(connT), ip(off), ip(cols), ip(sizes)) == 0
    Nc, nnz, n_con, n_ch = (int(v) for v in sizes)
    z = lambda n: np.zeros(n, dtype=np.int32)  # noqa: E731
    L = dict(par0=z(N), par1=z(N), r_off=z(Nc + 1), r_cols=z(nnz), ch_off=z(Nc + 1), ch=z(n_ch),
             ch_w=np.zeros(n_ch, dtype=np.float32), pos_off=z(n_ch + 1), con_pos=np.zeros(n_con, dtype=np.uint16))
    shim.rops_fetch(ip(L["par0"]), ip(L["par1"]), ip(L["r_off"]), ip(L["r_cols"]), ip(L["ch_off"]), ip(L["ch"]),
                    L["ch_w"].ctypes.data_as(C.POINTER(C.c_float)), ip(L["pos_off"]),
                    L["con_pos"].ctypes.data_as(C.POINTER(C.c_ushort)))
    L["long"] = {}
    for cap in (4, 16, 128):
        rows = z(Nc)
        n = shim.rops_long_rows(cap, ip(rows))
        L["long"][cap] = rows[:n].copy()
    L.update(X=X, conn=conn, off=off, cols=cols, Nc=Nc, n_con=n_con)
    _lists[name] = L
    return L


@pytest.mark.parametrize("name", MESHES)
def test_positions_are_the_search_in_the_row(shim, name):
    L = lists(shim, name)
    off, cols, r_off, r_cols, ch_off, ch, pos_off, con_pos = (L[k] for k in ("off", "cols", "r_off", "r_cols", "ch_off", "ch",
                                                                           "pos_off", "con_pos"))
    deg = np.diff(off)
    assert pos_off[0] == 0 and pos_off[-1] == L["n_con"] and np.array_equal(np.diff(pos_off), deg[ch])
    assert np.diff(r_off).max() < 65535                                  # nothing saturates on these meshes
    seen = 0
    for I in range(L["Nc"]):
        row = r_cols[r_off[I]:r_off[I + 1]]
        for t in range(ch_off[I], ch_off[I + 1]):
            i = ch[t]
            pos = con_pos[pos_off[t]:pos_off[t + 1]].astype(np.int64)
            fine_cols = cols[off[i]:off[i + 1]]
            assert np.array_equal(pos, np.searchsorted(row, fine_cols)), (I, i)
            assert np.array_equal(row[pos], fine_cols)                   # the column is in the row, at that place
            assert len(np.unique(pos)) == len(pos), (I, i)               # one lane per image element within a child
            seen += len(pos)
    assert seen == L["n_con"]


@pytest.mark.parametrize("name", MESHES)
def test_lists_reproduce_pt_h_of_the_oracle(shim, name):
    L = lists(shim, name)
    X, conn = L["X"], L["conn"]
    N, Nc = X.shape[0], L["Nc"]
    o = make_oracle(X, conn, MATERIALS["svk"], fixed_x0(X))
    ro, ci, val = o.assemble_hessian(1e-3, 1e14)
    off, cols = L["off"], L["cols"]
    assert np.array_equal(ro[::3], 9 * off)                              # the oracle's pattern is the node adjacency's
    assert np.array_equal(np.concatenate([ci[ro[3 * i]:ro[3 * i + 1]:3] // 3 for i in range(N)]), cols)
    H =sp.csr_matrix((val, ci, ro), shape=(3 * N, 3 * N))
    r_off, r_cols, ch_off, ch, ch_w, pos_off, con_pos = (L[k] for k in ("r_off", "r_cols", "ch_off", "ch", "ch_w", "pos_off",
                                                                      "con_pos"))
    # as the kernel runs them: image [blocks][9] per row, zero start, children ascending, entry (d, k, e) of the child's
    # row of H -- the 9 deg doubles from 9 off[i], [d][k][e] -- into image[con_pos[k]][3 d + e]
    out = np.zeros((len(r_cols), 9))
    for I in range(Nc):
        img = np.zeros((r_off[I + 1] - r_off[I], 9))
        for t in range(ch_off[I], ch_off[I + 1]):
            i = ch[t]
            deg = off[i + 1] - off[i]
            rows = val[9 * off[i]:9 * off[i] + 9 * deg].reshape(3, deg, 3)
            pos = con_pos[pos_off[t]:pos_off[t + 1]].astype(np.int64)
            for d in range(3):
                img[pos, 3 * d:3 * d + 3] += float(ch_w[t]) * rows[d]
        out[r_off[I]:r_off[I + 1]] = img
    dev = block_csr(r_off, r_cols, out, N)
    P = gn.prolongation(L["par0"], L["par1"], Nc)
    ref = (P.T @ H).tocsr()
    err = float(abs(dev - ref).max() / abs(ref).max())
    print(f"{name}: lists vs P^T H {err:.3e} x max |P^T H|, {L['n_con']} contributions, rows of {np.diff(r_off).min()}.."
          f"{np.diff(r_off).max()} blocks")
    assert err <= 1e-15


def block_csr(off, cols, blocks, n_fine):
    """node-block CSR with [blocks][3 d + e] values -> SciPy CSR of 3 Nc x 3 N"""
    nc = len(off) - 1
    brow = np.repeat(np.arange(nc), np.diff(off))
    r = (3 * brow[:, None, None] + np.arange(3)[None, :, None] + np.zeros((1, 1, 3), dtype=np.int64)).reshape(-1)
    c = (3 * cols.astype(np.int64)[:, None, None] + np.zeros((1, 3, 1), dtype=np.int64) + np.arange(3)[None, None, :]).reshape(-1)
    return sp.csr_matrix((blocks.reshape(-1), (r, c)), shape=(3 * nc, 3 * n_fine))


@pytest.mark.parametrize("name", MESHES)
def test_long_row_list_is_exact(shim, name):
    L = lists(shim, name)
    length = np.diff(L["r_off"])
    for cap in (4, 16, 128):
        assert np.array_equal(L["long"][cap], np.where(length > cap)[0]), cap
    print(name, "rows beyond 4 / 16 / 128 blocks:", [len(L["long"][c]) for c in (4, 16, 128)], "of", len(length))
    assert len(L["long"][4]) > 0                                         # the small capacities do split these meshes
