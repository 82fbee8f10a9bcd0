"""Host lists of the solve set-up from the element records (csrc/pmg_host.h: build_image_groups, image_mass_table) through a
small native shim, without a GPU.  The image row of coarse node I, sum over the children of w H[child, :], is assembled by
assemble_affine_kernel<.., COARSE> as the row of the vertex's linear hat function: one instance per (element, corner), lane n
adding the blocks of column "vertex n" and of the mid-edge columns (n, p) into the group's accumulator at the 16-bit words of
the lists, rows streamed out at 9 r_off[I] in H's row layout.  Checked on the meshes of tests/galerkin_np.py and on a single
element and two elements sharing a face:

  * every (element, corner) instance occurs exactly once, in the group of its vertex's row; every word lies inside the
    accumulator of its row and names the column it should; the two lanes of a mid-edge column agree; the rows' image offsets
    are a bijection onto [0, blocks of R);
  * the [4][16] mass table is cmass[c] + 1/2 sum over the three mid-edge nodes at c;
  * the lists executed in NumPy as the kernel executes them, on the element matrices h K_e + M_e / h of the oracle (which
    assemble to the oracle's H, asserted), plus the pinned-children list, reproduce sum_children w H[child, :] of the oracle's
    H within 1e-12 of the largest entry, the bound of tests/test_galerkin_rows_host.py;
  * the pinned-children list holds each child of each row once, with its weight and the position of its own column."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import orc
from tests import edge_meshes as em
from tests import galerkin_np as gn
from tests.helpers import MATERIALS, fixed_x0, make_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ["beam_3x2x1", "box", "permuted", "one_tet", "two_tets"]
EDGES = [(0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3)]                 # local mid-edge nodes 4..9
MID = {frozenset(e): 4 + k for k, e in enumerate(EDGES)}
H_STEP, RHO = 1e-3, 1e14
_lists = {}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("setup_records") / "libsetup_records_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "setup_records_shim.cc")])
    return C.CDLL(str(so))


def ptr(a, t=C.c_int):
    return a.ctypes.data_as(C.POINTER(t))


def mesh(name):
    if name == "one_tet":
        return em.one_tet()
    if name == "two_tets":
        return em.t10_from_tets([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.2, 0.9, 0.0], [0.1, 0.3, 0.8], [1.1, 0.9, 0.9]],
                                [[0, 1, 2, 3], [4, 1, 2, 3]])
    return gn.mesh(name)


def lists(shim, name, budgets=(48, 1536)):
    key = (name, budgets)
    if key in _lists:
        return _lists[key]
    X, conn = mesh(name)
    N, E = X.shape[0], conn.shape[0]
    off, cols = gn.node_adjacency(conn, N)
    off, cols = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    connT = np.ascontiguousarray(conn.T, dtype=np.int32)
    xyz = [np.ascontiguousarray(X[:, k], dtype=np.float64) for k in range(3)]
    sizes = np.zeros(8, dtype=np.int32)
    assert shim.sr_build(N, E, ptr(connT), ptr(off), ptr(cols), ptr(xyz[0], C.c_double), ptr(xyz[1], C.c_double),
                         ptr(xyz[2], C.c_double), budgets[0], budgets[1], ptr(sizes)) == 0
    Nc, nnz, n_ch, G, P, rows, n_inst, acc_max = (int(v) for v in sizes)
    z = lambda n: np.zeros(n, dtype=np.int32)  # noqa: E731
    L = dict(par0=z(N), par1=z(N), r_off=z(Nc + 1), r_cols=z(nnz), ch_off=z(Nc + 1), ch=z(n_ch),
             ch_w=np.zeros(n_ch, dtype=np.float32), ch_row=z(n_ch), ch_pos=z(n_ch), id_off=z(Nc + 1), id_ch=z(Nc),
             id_w=np.zeros(Nc, dtype=np.float32), id_pos=np.zeros(nnz, dtype=np.uint16), g_pass_off=z(G + 1), pt=z(4 * P),
             gr_info=z(4 * rows), gi_head=z(2 * n_inst), gi_ent=z(8 * n_inst))
    shim.sr_fetch_rows(ptr(L["par0"]), ptr(L["par1"]), ptr(L["r_off"]), ptr(L["r_cols"]), ptr(L["ch_off"]), ptr(L["ch"]),
                       ptr(L["ch_w"], C.c_float), ptr(L["ch_row"]), ptr(L["ch_pos"]), ptr(L["id_off"]), ptr(L["id_ch"]),
                       ptr(L["id_w"], C.c_float), ptr(L["id_pos"], C.c_ushort))
    shim.sr_fetch_groups(ptr(L["g_pass_off"]), ptr(L["pt"]), ptr(L["gr_info"]), ptr(L["gi_head"]), ptr(L["gi_ent"]))
    L.update(X=X, conn=conn, off=off, cols=cols, Nc=Nc, nnz=nnz, G=G, P=P, rows=rows, n_inst=n_inst, acc_max=acc_max,
             pt=L["pt"].reshape(-1, 4), gr_info=L["gr_info"].reshape(-1, 4), gi_head=L["gi_head"].reshape(-1, 2),
             gi_ent=L["gi_ent"].reshape(-1, 4, 2))
    _lists[key] = L
    return L


def words(ent):
    """the four 16-bit words of one (instance, lane): accumulator offset / 3 of the block (n, p), p = 0..3"""
    a, b = int(ent[0]) & 0xffffffff, int(ent[1]) & 0xffffffff
    return [a & 0xffff, a >> 16, b & 0xffff, b >> 16]


def groups(L):
    """per group: (rows [(acc offset, image block offset, deg, coarse row)], instances [index])"""
    out = []
    for g in range(L["G"]):
        p0, p1 = L["g_pass_off"][g], L["g_pass_off"][g + 1]
        first = L["pt"][p0]
        assert first[1] & 32 and L["pt"][p1 - 1][1] & 64                 # first / last flags frame the group
        nrows, r0 = first[1] >> 8, first[2]
        rows = [(int(i[0]) & 0xffff, int(i[1]), int(i[2]), int(i[3])) for i in L["gr_info"][r0:r0 + nrows]]
        inst = []
        for p in range(p0, p1):
            start, cnt = int(L["pt"][p][0]), int(L["pt"][p][1]) & 31
            assert cnt <= 16 and (L["pt"][p][1] >> 8) == nrows and L["pt"][p][2] == r0 and L["pt"][p][3] == first[3]
            inst += list(range(start, start + cnt))
        out.append((rows, inst, int(first[3])))
    return out


@pytest.mark.parametrize("name", MESHES)
def test_every_corner_instance_once_words_inside_the_accumulator_offsets_a_bijection(shim, name):
    L = lists(shim, name)
    conn, par0, r_off, r_cols = L["conn"], L["par0"], L["r_off"], L["r_cols"]
    E = conn.shape[0]
    assert L["n_inst"] == 4 * E and L["rows"] == L["Nc"]
    seen_inst, seen_rows, blocks = [], [], 0
    for rows, inst, acc_n in groups(L):
        assert acc_n <= L["acc_max"] < 65536
        a_end = 0
        for a0, off0, deg, I in rows:                                    # the rows tile the accumulator, in order
            assert a0 == a_end and off0 == r_off[I] and deg == r_off[I + 1] - r_off[I]
            a_end = a0 + 9 * deg
            seen_rows.append(I)
            blocks += deg
        assert a_end == acc_n
        by_row = {I: (a0, deg) for a0, _, deg, I in rows}
        for w in inst:
            code, stride = (int(v) for v in L["gi_head"][w])
            e, c = divmod(code, 10)
            assert c < 4                                                 # corners only
            I = int(par0[conn[e, c]])
            assert I in by_row                                           # in the group of its vertex's row
            a0, deg = by_row[I]
            assert stride == 3 * deg
            row_cols = r_cols[r_off[I]:r_off[I + 1]]
            ws = [words(L["gi_ent"][w][n]) for n in range(4)]
            for n in range(4):
                for p in range(4):
                    j = n if p == n else MID[frozenset((n, p))]
                    pos = ws[n][p] - a0 // 3
                    assert 0 <= pos < deg and row_cols[pos] == conn[e, j], (w, n, p)
                    assert ws[n][p] == ws[p][n] or p == n                 # the two lanes of a mid-edge column agree
            seen_inst.append(code)
    assert sorted(seen_inst) == sorted(10 * e + c for e in range(E) for c in range(4))      # every instance exactly once
    assert sorted(seen_rows) == list(range(L["Nc"])) and blocks == L["nnz"]                # offsets: a bijection onto R's blocks
    # ascending element inside a row: the order of the sum
    order = {}
    for _, inst, _ in groups(L):
        for w in inst:
            e, c = divmod(int(L["gi_head"][w][0]), 10)
            order.setdefault(int(par0[conn[e, c]]), []).append(e)
    assert all(v == sorted(v) for v in order.values())


@pytest.mark.parametrize("budgets", [(16, 600), (32, 1024), (48, 1536), (64, 3000)])
def test_budgets_are_parameters_and_fill_the_passes(shim, budgets):
    L = lists(shim, "box", budgets)
    per_group = [len(inst) for _, inst, _ in groups(L)]
    assert sum(per_group) == L["n_inst"]
    fill = L["n_inst"] / (16.0 * L["P"])
    print(f"box, budgets {budgets}: {L['G']} groups, {L['P']} passes, filled to {fill:.2f}, accumulator {L['acc_max']} doubles")
    single = max(9 * int(d) for d in np.diff(L["r_off"]))
    assert L["acc_max"] <= max(budgets[1], single)                       # a row beyond the budget is a group of its own


def test_the_coarse_mass_table(shim):
    cm = np.random.default_rng(5).normal(size=(10, 16))
    cm4 = np.zeros((4, 16))
    shim.sr_mass_table(ptr(cm, C.c_double), ptr(cm4, C.c_double))
    for c in range(4):
        want = cm[c] + 0.5 * sum(cm[MID[frozenset((c, p))]] for p in range(4) if p != c)
        assert np.allclose(cm4[c], want, rtol=0, atol=4 * np.finfo(float).eps * np.abs(cm).max())


def element_matrices(o, rho0):
    """[E, 10, 10, 3, 3]: h K_e + M_e / h, the element's share of the oracle's H without the pinned rows' penalty"""
    Ke, _ = o.element_tangents()
    E = o.E
    qx, qy, qz, qw = orc.keast5()
    Lq = np.stack([1.0 - qx - qy - qz, qx, qy, qz], axis=1)              # [5, 4]
    Nq = np.concatenate([Lq * (2.0 * Lq - 1.0), np.stack([4.0 * Lq[:, a] * Lq[:, b] for a, b in EDGES], axis=1)], axis=1)
    Cm = np.einsum("q,qi,qj->ij", qw, Nq, Nq)
    He = H_STEP * Ke.reshape(E, 10, 3, 10, 3).transpose(0, 1, 3, 2, 4).copy()
    He += (rho0 / H_STEP) * o.detJ[:, 0][:, None, None, None, None] * Cm[None, :, :, None, None] * np.eye(3)[None, None, None]
    return He


@pytest.mark.parametrize("name", MESHES)
def test_lists_reproduce_the_weighted_rows_of_the_oracle_s_h(shim, name):
    L = lists(shim, name)
    X, conn = L["X"], L["conn"]
    N, Nc, E = X.shape[0], L["Nc"], conn.shape[0]
    fixed = fixed_x0(X) if name not in ("one_tet", "two_tets") else np.array([0, int(conn[0, 4]), int(conn[0, 6])], dtype=np.int32)
    m = MATERIALS["svk"]
    o = make_oracle(X, conn, m, fixed)
    ro, ci, val = o.assemble_hessian(H_STEP, RHO)
    H = sp.csr_matrix((val, ci, ro), shape=(3 * N, 3 * N))
    He = element_matrices(o, m["rho0"])
    # the element matrices assemble to the oracle's H (without the penalty): what the lists run on is the oracle's
    rows = (3 * conn[:, :, None, None, None] + np.arange(3)[None, None, None, :, None]) + 0 * conn[:, None, :, None, None]
    colsx = (3 * conn[:, None, :, None, None] + np.arange(3)[None, None, None, None, :]) + 0 * conn[:, :, None, None, None]
    A = sp.csr_matrix((He.reshape(-1), (np.broadcast_to(rows, He.shape).reshape(-1), np.broadcast_to(colsx, He.shape).reshape(-1))),
                      shape=(3 * N, 3 * N))
    pen = np.zeros(3 * N)
    pen[(3 * fixed[:, None] + np.arange(3)).reshape(-1)] = H_STEP * H_STEP * RHO
    assert abs(A + sp.diags(pen) - H).max() <= 1e-12 * abs(H).max()
    # the lists, as the kernel runs them
    image = np.full(9 * L["nnz"], np.nan)
    for grows, inst, acc_n in groups(L):
        acc = np.zeros(acc_n)
        for w in inst:
            code, stride = (int(v) for v in L["gi_head"][w])
            e, c = divmod(code, 10)
            hat = He[e, c] + 0.5 * sum(He[e, MID[frozenset((c, p))]] for p in range(4) if p != c)      # [10, 3, 3]: row of L_c
            for n in range(4):
                ws = words(L["gi_ent"][w][n])
                for r in range(3):
                    if r == 2 and n >= 2:
                        break
                    p = (n + r) & 3
                    j = n if r == 0 else MID[frozenset((n, p))]
                    for rr in range(3):
                        acc[3 * ws[p] + rr * stride:3 * ws[p] + rr * stride + 3] += hat[j, rr]
        for a0, off0, deg, _ in grows:
            image[9 * off0:9 * off0 + 9 * deg] = acc[a0:a0 + 9 * deg]
    assert np.all(np.isfinite(image))                                    # every block of the image was written
    pinned = np.zeros(N, dtype=bool)
    pinned[fixed] = True
    for t in np.nonzero(pinned[L["ch"]])[0]:                             # the pinned children's penalties
        I = L["ch_row"][t]
        length = L["r_off"][I + 1] - L["r_off"][I]
        for d in range(3):
            image[9 * L["r_off"][I] + d * 3 * length + 3 * L["ch_pos"][t] + d] += float(L["ch_w"][t]) * H_STEP * H_STEP * RHO
    T = (gn.prolongation(L["par0"], L["par1"], Nc).T @ H).tocsr()
    err = float(abs(gn.dof_csr(L["r_off"], L["r_cols"], image, n_cols=N) - T).max() / abs(T).max())
    print(f"{name}: image rows from the lists vs sum_children w H[child, :] {err:.3e} x max, {L['G']} groups, {L['P']} passes")
    assert err <= 1e-12


@pytest.mark.parametrize("name", MESHES)
def test_children_list_and_the_one_child_tables(shim, name):
    L = lists(shim, name)
    r_off, r_cols, ch_off, ch = L["r_off"], L["r_cols"], L["ch_off"], L["ch"]
    par0, par1 = L["par0"], L["par1"]
    pairs = set()
    for I in range(L["Nc"]):
        for t in range(ch_off[I], ch_off[I + 1]):
            i = int(ch[t])
            assert L["ch_row"][t] == I and (par0[i] == I or par1[i] == I)
            assert L["ch_w"][t] == (1.0 if par0[i] == par1[i] else 0.5)
            assert r_cols[r_off[I] + L["ch_pos"][t]] == i                 # its own column in the row
            pairs.add((I, i))
    want = {(int(p), i) for i in range(len(par0)) for p in {par0[i], par1[i]}}
    assert pairs == want and len(pairs) == len(ch)                       # each child of each row once
    assert np.array_equal(L["id_off"], np.arange(L["Nc"] + 1)) and np.array_equal(L["id_ch"], np.arange(L["Nc"]))
    assert np.all(L["id_w"] == 1.0)
    for I in range(L["Nc"]):
        assert np.array_equal(L["id_pos"][r_off[I]:r_off[I + 1]], np.arange(r_off[I + 1] - r_off[I]))
