"""Host lists of the vertex-level Galerkin operator summed from the row image of R (csrc/pmg_host.h: GalRowsHost next to
RopHost) through a small native shim, without a GPU.  The kernel (csrc/solver_kernels.hip pmg_galerkin_row) builds the image
T[I, :] = (P^T H)[I, :] of a coarse row as the streamed build of R does -- zero start, children in ascending fine id, one
fma(w_i, H, image) per contribution at the position con_pos gives -- and then sums every block (I, J), J >= I, of
Hc = P^T H P from it: acc = fma(w, T[I, b], acc) from zero over the block's terms in ascending position b, w = 1 or 1/2, stored
at its place and, off the diagonal, transposed at c_mirror.  Checked on the meshes of tests/galerkin_np.py:

  * every term's position lies inside the R row of its block, positions ascend strictly within a block, the weight bit says
    1 exactly where the fine column is the vertex J itself;
  * per coarse row every (position, parent J >= I) pair occurs in exactly one list, and no pair with J < I occurs;
  * the lists executed in NumPy exactly as the kernel executes them (the weights are powers of two, so fma(w, x, acc) is
    acc + w x rounded once, which is what NumPy computes) reproduce SciPy's P^T H P of the oracle's H to 1e-12 x max |Hc|,
    the bound of tests/test_gpu_setup_kernels.py, with an off-diagonal asymmetry of exactly 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import galerkin_np as gn
from tests import galerkin_rows_np as grn
from tests.helpers import MATERIALS, fixed_x0, make_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ["beam_3x2x1", "box", "permuted"]
_lists = {}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("galr") / "libgalerkin_rows_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "galerkin_rows_shim.cc")])
    return C.CDLL(str(so))


def ptr(a, t=C.c_int):
    return a.ctypes.data_as(C.POINTER(t))


def lists(shim, name):
    """the shim holds one build at a time: build, copy everything out, keep it"""
    if name in _lists:
        return _lists[name]
    X, conn = gn.mesh(name)
    N, E = X.shape[0], conn.shape[0]
    off, cols = gn.node_adjacency(conn, N)
    off, cols = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    connT = np.ascontiguousarray(conn.T, dtype=np.int32)                # column-major [10][E]
    sizes = np.zeros(7, dtype=np.int32)
    assert shim.galr_build(N, E, ptr(connT), ptr(off), ptr(cols), ptr(sizes)) == 0
    Nc, nnz, n_con, n_ch, nnz_c, n_upper, n_term = (int(v) for v in sizes)
    z = lambda n: np.zeros(n, dtype=np.int32)  # noqa: E731
    L = dict(par0=z(N), par1=z(N), r_off=z(Nc + 1), r_cols=z(nnz), ch_off=z(Nc + 1), ch=z(n_ch),
             ch_w=np.zeros(n_ch, dtype=np.float32), pos_off=z(n_ch + 1), con_pos=np.zeros(n_con, dtype=np.uint16),
             c_off=z(Nc + 1), c_cols=z(nnz_c), cblk_row=z(nnz_c), c_upper=z(n_upper), c_mirror=z(nnz_c), row_off=z(Nc + 1),
             term_off=z(n_upper + 1), term_pos=np.zeros(n_term, dtype=np.uint16), term_w=np.zeros(n_term, dtype=np.uint8))
    shim.galr_fetch_rows(ptr(L["par0"]), ptr(L["par1"]), ptr(L["r_off"]), ptr(L["r_cols"]), ptr(L["ch_off"]), ptr(L["ch"]),
                         ptr(L["ch_w"], C.c_float), ptr(L["pos_off"]), ptr(L["con_pos"], C.c_ushort))
    shim.galr_fetch_combine(ptr(L["c_off"]), ptr(L["c_cols"]), ptr(L["cblk_row"]), ptr(L["c_upper"]), ptr(L["c_mirror"]),
                            ptr(L["row_off"]), ptr(L["term_off"]), ptr(L["term_pos"], C.c_ushort), ptr(L["term_w"], C.c_ubyte))
    L.update(X=X, conn=conn, off=off, cols=cols, Nc=Nc, n_upper=n_upper, n_term=n_term)
    _lists[name] = L
    return L


@pytest.mark.parametrize("name", MESHES)
def test_terms_lie_in_their_row_ascend_and_weigh_one_or_a_half(shim, name):
    L = lists(shim, name)
    r_off, r_cols, row_off, term_off, term_pos, term_w = (L[k] for k in ("r_off", "r_cols", "row_off", "term_off", "term_pos",
                                                                        "term_w"))
    par0, par1, c_upper, c_cols, cblk_row = (L[k] for k in ("par0", "par1", "c_upper", "c_cols", "cblk_row"))
    assert row_off[0] == 0 and row_off[-1] == L["n_upper"] and term_off[0] == 0 and term_off[-1] == L["n_term"]
    assert set(np.unique(term_w)) <= {0, 1}                              # the weight bit: 1 -> 1, 0 -> 1/2
    for I in range(L["Nc"]):
        length = r_off[I + 1] - r_off[I]
        us = np.arange(row_off[I], row_off[I + 1])
        assert len(us) >= 1 and np.all(cblk_row[c_upper[us]] == I)       # the row's upper blocks, and they are this row's
        assert c_cols[c_upper[us[0]]] == I                               # the diagonal block first: the kernel scales with it
        assert np.all(np.diff(c_cols[c_upper[us]]) > 0)
        for u in us:
            J = c_cols[c_upper[u]]
            pos = term_pos[term_off[u]:term_off[u + 1]].astype(np.int64)
            assert len(pos) >= 1 and pos.min() >= 0 and pos.max() < length, (I, J)
            assert np.all(np.diff(pos) > 0), (I, J)                      # ascending: the order of the sum
            j = r_cols[r_off[I] + pos]
            assert np.all((par0[j] == J) | (par1[j] == J)), (I, J)       # every term's fine column has J among its parents
            assert np.array_equal(term_w[term_off[u]:term_off[u + 1]], (par0[j] == par1[j]).astype(np.uint8)), (I, J)


@pytest.mark.parametrize("name", MESHES)
def test_every_position_parent_pair_is_in_exactly_one_list(shim, name):
    L = lists(shim, name)
    r_off, r_cols, row_off, term_off, term_pos = (L[k] for k in ("r_off", "r_cols", "row_off", "term_off", "term_pos"))
    par0, par1, c_upper, c_cols = (L[k] for k in ("par0", "par1", "c_upper", "c_cols"))
    seen = 0
    for I in range(L["Nc"]):
        j = r_cols[r_off[I]:r_off[I + 1]]
        b = np.arange(len(j))
        want = set(zip(b[par0[j] >= I].tolist(), par0[j][par0[j] >= I].tolist()))
        two = (par1[j] != par0[j]) & (par1[j] >= I)
        want |= set(zip(b[two].tolist(), par1[j][two].tolist()))
        have = []
        for u in range(row_off[I], row_off[I + 1]):
            J = int(c_cols[c_upper[u]])
            assert J >= I                                                # the lower triangle is never summed
            have += [(int(p), J) for p in term_pos[term_off[u]:term_off[u + 1]]]
        assert len(have) == len(set(have)), I                            # no pair twice
        assert set(have) == want, I                                      # every pair once, none with J < I, none foreign
        seen += len(have)
    assert seen == L["n_term"]


def run_rows(L, val):
    """the lists on H's values (DOF-level layout) exactly as the kernel runs them: Hc in the DOF-level layout"""
    off, r_off, ch_off, ch, ch_w, pos_off, con_pos = (L[k] for k in ("off", "r_off", "ch_off", "ch", "ch_w", "pos_off", "con_pos"))
    c_off, c_upper, c_mirror, cblk_row = (L[k] for k in ("c_off", "c_upper", "c_mirror", "cblk_row"))
    row_off, term_off, term_pos, term_w = (L[k] for k in ("row_off", "term_off", "term_pos", "term_w"))
    Hc = np.full(9 * len(L["c_cols"]), np.nan)
    deg_c = np.diff(c_off)
    d, e = np.divmod(np.arange(9), 3)
    for I in range(L["Nc"]):
        img = np.zeros((r_off[I + 1] - r_off[I], 9))                     # the image: zero start, children ascending
        for t in range(ch_off[I], ch_off[I + 1]):
            i = ch[t]
            deg = off[i + 1] - off[i]
            rows = val[9 * off[i]:9 * off[i] + 9 * deg].reshape(3, deg, 3)
            pos = con_pos[pos_off[t]:pos_off[t + 1]].astype(np.int64)
            for dd in range(3):
                img[pos, 3 * dd:3 * dd + 3] += float(ch_w[t]) * rows[dd]
        for u in range(row_off[I], row_off[I + 1]):                      # the combine: one chain per entry, ascending position
            acc = np.zeros(9)
            for t in range(term_off[u], term_off[u + 1]):
                acc = acc + (1.0 if term_w[t] else 0.5) * img[term_pos[t]]
            cb = c_upper[u]
            Hc[9 * c_off[I] + d * 3 * deg_c[I] + 3 * (cb - c_off[I]) + e] = acc
            cm = c_mirror[cb]
            if cm != cb:                                                 # the mirror store, transposed
                J = cblk_row[cm]
                Hc[9 * c_off[J] + e * 3 * deg_c[J] + 3 * (cm - c_off[J]) + d] = acc
    return Hc


@pytest.mark.parametrize("name", MESHES)
def test_lists_reproduce_pt_h_p_of_the_oracle(shim, name):
    L = lists(shim, name)
    X, conn = L["X"], L["conn"]
    N, Nc = X.shape[0], L["Nc"]
    o = make_oracle(X, conn, MATERIALS["svk"], fixed_x0(X))
    ro, ci, val = o.assemble_hessian(1e-3, 1e14)
    assert np.array_equal(ro[::3], 9 * L["off"])                         # the oracle's pattern is the node adjacency's
    H = sp.csr_matrix((val, ci, ro), shape=(3 * N, 3 * N))
    Hc = run_rows(L, val)
    assert np.all(np.isfinite(Hc))                                       # every block of Hc was stored
    dev = gn.dof_csr(L["c_off"], L["c_cols"], Hc)
    P = gn.prolongation(L["par0"], L["par1"], Nc)
    ref = (P.T @ H @ P).tocsr()
    err = float(abs(dev - ref).max() / abs(ref).max())
    asym = grn.off_diagonal_asymmetry(L["c_off"], L["c_cols"], Hc)
    print(f"{name}: row lists vs P^T H P {err:.3e} x max |Hc|, off-diagonal asymmetry {asym:.1e}, {L['n_term']} terms in "
          f"{L['n_upper']} blocks")
    assert err <= 1e-12
    assert asym == 0.0
