"""Host set-up of the restricted fine operator R = S_c P^T S_f^-1 Hs (csrc/pmg_host.h pmg_restrict_op_build) through a
small native shim: the pattern is that of P^T pattern(H), columns ascend, and every (child, fine block) pair feeds exactly
one block of R exactly once, children in ascending fine id."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import load_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("rop") / "librestrict_op_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "restrict_op_shim.cc")])
    return C.CDLL(str(so))


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


@pytest.mark.parametrize("tag", ["beam_3x2x1", "res2", "bunny"])
def test_pattern_and_contribution_lists(shim, tag):
    X, conn = load_mesh(tag)
    N, E = X.shape[0], conn.shape[0]
    inc = sp.csr_matrix((np.ones(10 * E), (np.repeat(np.arange(E), 10), conn.reshape(-1))), shape=(E, N))
    A = (inc.T @ inc).tocsr()
    A.sort_indices()
    off, cols = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    connT = np.ascontiguousarray(conn.T, dtype=np.int32)                # column-major [10][E]
    sizes = np.zeros(4, dtype=np.int32)
    assert shim.rop_build(N, E, ip(connT), ip(off), ip(cols), ip(sizes)) == 0
    Nc, nnz, n_con, n_ch = (int(v) for v in sizes)
    par0, par1 = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    r_off, r_cols = np.zeros(Nc + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32)
    ch_off, ch, ch_w = np.zeros(Nc + 1, dtype=np.int32), np.zeros(n_ch, dtype=np.int32), np.zeros(n_ch, dtype=np.float32)
    con_off, con_blk, con_ord = np.zeros(nnz + 1, dtype=np.int32), np.zeros(n_con, dtype=np.int32), np.zeros(n_con, dtype=np.uint8)
    shim.rop_fetch(ip(par0), ip(par1), ip(r_off), ip(r_cols), ip(ch_off), ip(ch), ch_w.ctypes.data_as(C.POINTER(C.c_float)),
                   ip(con_off), ip(con_blk), con_ord.ctypes.data_as(C.POINTER(C.c_ubyte)))
    # the pattern of P^T pattern(H), node level
    has = np.arange(N)
    Pn = sp.csr_matrix((np.ones(2 * N), (np.concatenate([has, has]), np.concatenate([par0, par1]))), shape=(N, Nc))
    ref = (Pn.T @ sp.csr_matrix((np.ones(len(cols)), cols, off), shape=(N, N))).tocsr()
    ref.sort_indices()
    assert np.array_equal(r_off, ref.indptr) and np.array_equal(r_cols, ref.indices)
    for I in range(Nc):
        assert np.all(np.diff(r_cols[r_off[I]:r_off[I + 1]]) > 0)       # ascending, no duplicates
    # children: ascending fine id, weights 1 (the vertex) or 1/2 (mid-edge nodes), every parent link once
    assert n_ch == int(np.sum(par0 == par1) + 2 * np.sum(par0 != par1))
    for I in range(Nc):
        c = ch[ch_off[I]:ch_off[I + 1]]
        assert np.all(np.diff(c) > 0) and len(c) <= 256
        assert np.all((par0[c] == I) | (par1[c] == I))
        assert np.array_equal(ch_w[ch_off[I]:ch_off[I + 1]], np.where(par0[c] == par1[c], 1.0, 0.5).astype(np.float32))
    # contributions: block b of row I takes fine block g of child ch[ch_off[I] + ord]; the column is the block's own
    assert con_off[0] == 0 and con_off[-1] == n_con and np.all(np.diff(con_off) >= 1)
    b_of = np.repeat(np.arange(nnz), np.diff(con_off))
    I_of = np.repeat(np.arange(Nc), np.diff(r_off))[b_of]
    child = ch[ch_off[I_of] + con_ord]
    f_row = np.repeat(np.arange(N), np.diff(off))
    assert np.array_equal(f_row[con_blk], child)                          # the fine block lies in that child's row
    assert np.array_equal(cols[con_blk], r_cols[b_of])                    # and in the block's column
    for b in np.where(np.diff(con_off) > 1)[0]:
        assert np.all(np.diff(child[con_off[b]:con_off[b + 1]]) > 0)      # ascending child order inside a block
    # every (parent, fine block) pair exactly once
    pairs = I_of.astype(np.int64) * len(cols) + con_blk
    assert len(np.unique(pairs)) == n_con
    want = np.concatenate([par0[f_row].astype(np.int64) * len(cols) + np.arange(len(cols)),
                           (par1[f_row].astype(np.int64) * len(cols) + np.arange(len(cols)))[par0[f_row] != par1[f_row]]])
    assert np.array_equal(np.sort(pairs), np.sort(want))
