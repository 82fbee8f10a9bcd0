"""The merged V-cycle (restriction through R = S_c P^T S_f^-1 Hs, tests/restricted_op_np.py) against the present cycle
(tests/precond_np.py) on H from the oracle: beam_3x2x1, res2 and bunny, ks = 1, 2, 4, fine storage 16 and 32 bits.

  * fp64 work vectors: the same operator to 1e-13 of ||z|| (eps x ~1e2 operations per entry, with margin);
  * fp32 work vectors and R rounded to fp32: within 8 x the fp32 floor of the present cycle (the floor as
    tests/test_gpu_precond_operator.py computes it: present cycle in float32 against float64, same matrix rounding);
  * R rounded to fp16: beyond that bound -- fp16(P^T Hs) != P^T fp16(Hs), which is why R is stored in 32 bits."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import precond_np as pn
from tests import restricted_op_np as rn
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_oracle

EDGES = [(0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3)]
_CACHE = {}


def problem(tag):
    """H at a perturbed state (x = 0 pinned where the mesh has such nodes), the vertex hierarchy, a third level of 4 bins"""
    if tag in _CACHE:
        return _CACHE[tag]
    X, conn = load_mesh(tag)
    fixed = fixed_x0(X)
    o = make_oracle(X, conn, MATERIALS["svk"], fixed)
    x = X + np.random.default_rng(7).normal(0.0, 1e-4, X.shape)
    x[fixed] = X[fixed]
    o.x, o.y, o.z = (np.ascontiguousarray(x[:, i]) for i in range(3))
    ro, ci, val = o.assemble_hessian(1e-3, 1e14)
    N = X.shape[0]
    H = sp.csr_matrix((val, ci, ro), shape=(3 * N, 3 * N))
    verts = np.unique(conn[:, :4])
    cid = -np.ones(N, dtype=np.int64)
    cid[verts] = np.arange(len(verts))
    par0, par1 = cid.copy(), cid.copy()
    for m, (a, b) in enumerate(EDGES):
        par0[conn[:, 4 + m]], par1[conn[:, 4 + m]] = cid[conn[:, a]], cid[conn[:, b]]
    P = pn.prolongation_p(par0, par1, len(verts))
    Hc = (P.T @ H @ P).tocsr()
    Xv = X[verts]
    t = (Xv[:, 0] - Xv[:, 0].min()) / (np.ptp(Xv[:, 0]) + 1e-9)
    agg = np.minimum((t * 4).astype(np.int64), 3)
    rvec = Xv - np.stack([Xv[agg == A].mean(axis=0) for A in range(4)])[agg]
    P2 = pn.prolongation_rbm(agg, rvec, 4)
    H3 = pn.level3_matrix(Hc, P2, np.ones(4, dtype=np.int64))
    rng = np.random.default_rng(11)
    vecs = [rng.normal(size=3 * N) for _ in range(3)]
    e = np.zeros(3 * N)
    e[3 * int(np.argmax(np.diff(ro)[::3])) + 1] = 1.0       # an impulse on the longest row
    _CACHE[tag] = dict(H=H, P=P, Hc=Hc, P2=P2, H3=H3, n=3 * N, vecs=vecs + [e], lam={})
    return _CACHE[tag]


def lam_max(p, name, level):
    """1.15 x the largest eigenvalue of (S D S)^-1 Hs (ARPACK; the levels are too large for dense eigenvalues)"""
    if name not in p["lam"]:
        Dinv = sp.block_diag(list(level.Dinv.astype(np.float64)), format="csr")
        A = (Dinv @ level.Hs.astype(np.float64)).tocsr()
        v0 = np.ones(A.shape[0])
        p["lam"][name] = 1.15 * float(np.max(spla.eigs(A, k=1, which="LM", v0=v0, tol=1e-6, return_eigenvectors=False).real))
    return p["lam"][name]


def states(p, store, ks):
    f, c, l3 = pn.Level(p["H"], store), pn.Level(p["Hc"], store), pn.Level(p["H3"], store)
    lf, lc, l33 = lam_max(p, "f%d" % store, f), lam_max(p, "c%d" % store, c), lam_max(p, "3_%d" % store, l3)
    kappa_s = 8.0 if ks <= 2 else 1.5 * ks * ks
    fine_pairs = pn.chebyshev_pairs(lf, kappa_s, ks)
    two = pn.cycle_state(fine_pairs, pn.chebyshev_pairs(lc, 216.0, 12))
    three = pn.cycle_state(fine_pairs, pn.chebyshev_pairs(lc, 90.0, 6), pn.chebyshev_pairs(l33, 96.0, 8))
    return two, three


def cycles(p, store, state, levels, dtype, merged, store_r=32):
    f, c = pn.Level(p["H"], store, dtype), pn.Level(p["Hc"], store, dtype)
    if levels == 2:
        return rn.two_level_cycle(f, c, p["P"], state, store_r) if merged else pn.two_level_cycle(f, c, p["P"], state)
    l3 = pn.Level(p["H3"], store, dtype)
    if merged:
        return rn.three_level_cycle(f, c, l3, p["P"], p["P2"], state, store_r)
    return pn.three_level_cycle(f, c, l3, p["P"], p["P2"], state)


def worst(op, ref_z, vecs):
    return max(float(np.linalg.norm(op(r) - z) / np.linalg.norm(z)) for r, z in zip(vecs, ref_z))


@pytest.mark.parametrize("store", [16, 32])
@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("tag", ["beam_3x2x1", "res2", "bunny"])
def test_merged_cycle_is_the_present_cycle(tag, ks, store):
    p = problem(tag)
    two, three = states(p, store, ks)
    for levels, st in ((2, two), (3, three)):
        ref = cycles(p, store, st, levels, np.float64, merged=False)
        z_ref = [ref(r) for r in p["vecs"]]
        # exact arithmetic: the same operator
        e64 = worst(cycles(p, store, st, levels, np.float64, merged=True, store_r=64), z_ref, p["vecs"])
        # the fp32 floor of the present cycle, and the merged cycle in the same arithmetic with R in 32 and in 16 bits
        floor = worst(cycles(p, store, st, levels, np.float32, merged=False), z_ref, p["vecs"])
        e32 = worst(cycles(p, store, st, levels, np.float32, merged=True, store_r=32), z_ref, p["vecs"])
        e16 = worst(cycles(p, store, st, levels, np.float32, merged=True, store_r=16), z_ref, p["vecs"])
        bound = min(8.0 * floor, 1e-3)
        print("%-10s ks %d store %d levels %d: fp64 %.1e  floor %.1e  bound %.1e  R fp32 %.1e  R fp16 %.1e"
              % (tag, ks, store, levels, e64, floor, bound, e32, e16))
        assert e64 <= 1e-13, (levels, e64)
        assert e32 <= bound, (levels, e32, bound)
        assert e16 > bound, (levels, e16, bound)


@pytest.mark.parametrize("tag", ["beam_3x2x1", "res2"])
def test_merged_cycle_is_symmetric(tag):
    """fp64 work vectors, R in 32 bits: the symmetry defect stays at the rounding of R (one fp32 rounding per entry)"""
    p = problem(tag)
    two, _ = states(p, 16, 2)
    op = cycles(p, 16, two, 2, np.float64, merged=True, store_r=32)
    a, b = p["vecs"][0], p["vecs"][1]
    za, zb = op(a), op(b)
    assert abs(a @ zb - b @ za) / (np.linalg.norm(a) * np.linalg.norm(zb)) <= 1e-6


def test_blockwise_definition_matches_the_matrix_product():
    """rn.restricted_operator_blocks (what the GPU test compares the device's R with) against the sparse triple product"""
    p = problem("beam_3x2x1")
    f, c = pn.Level(p["H"], 16), pn.Level(p["Hc"], 16)
    Hs = sp.csr_matrix(f.Hs)
    N = p["n"] // 3
    Pn = p["P"][::3, ::3].tocsr()
    par = [Pn.indices[Pn.indptr[i]:Pn.indptr[i + 1]] for i in range(N)]
    par0 = np.array([q.min() for q in par]); par1 = np.array([q.max() for q in par])
    A = sp.csr_matrix((np.ones(Hs.nnz), Hs.indices // 3, Hs.indptr))[::3].tocsr()
    A.sum_duplicates(); A.sort_indices()
    f_off, f_cols = A.indptr, A.indices
    rows = np.repeat(np.arange(N), np.diff(f_off))
    dense = Hs.toarray()
    f_vals = np.stack([dense[3 * i:3 * i + 3, 3 * j:3 * j + 3] for i, j in zip(rows, f_cols)])
    off, cols, vals, mags = rn.restricted_operator_blocks(f_off, f_cols, f_vals, f.sc, c.sc, par0, par1)
    R = rn.restricted_operator(f, c, p["P"], 64).toarray()
    got = np.zeros_like(R)
    for I in range(len(off) - 1):
        for k in range(off[I], off[I + 1]):
            got[3 * I:3 * I + 3, 3 * cols[k]:3 * cols[k] + 3] = vals[k]
    assert np.abs(got - R).max() <= 1e-14 * np.abs(R).max()
    assert np.all(np.abs(vals) <= mags * (1 + 1e-12) + 1e-300)
