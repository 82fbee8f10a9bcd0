"""The V-cycle that restricts the fine residual through the stored operator R = S_c P^T S_f^-1 Hs, restated in numpy next
to tests/precond_np.py (imported, not edited).  The present cycle forms res_B = res_A - Hs d_last in a pass of its own and
restricts it; the residual is linear in the direction, so

    r^_c = S_c P^T S_f^-1 res_A - R d_last ,   d := d_last + corr ,   restart pass: res_A - Hs (d_last + corr)

is the same operator in exact arithmetic.  R is built from the fine level's STORED (rounded) copy and rounded once through
`store_r` (32 on the device; 16 is here to show why it must not be)."""
import numpy as np
import scipy.sparse as sp

from tests import precond_np as pn


def restricted_operator(fine, coarse, P, store_r=32):
    """R = S_c P^T S_f^-1 Hs (Hs as the level holds it), entries rounded through store_r, in the work type of the level"""
    Hs = sp.csr_matrix(fine.Hs, dtype=np.float64)
    R = (sp.diags(coarse.sc) @ P.T @ sp.diags(1.0 / fine.sc) @ Hs).tocsr()
    R.data = pn.round_store(R.data, store_r)
    return R.astype(fine.dtype)


def _merged_cycle_hat(level, rhat, coef, terms, o_restart, R, restrict, coarse_solve, prolong):
    """the fine level of the merged cycle in the scaled space: `terms` pre-smoothing terms, the coarse right-hand side from
    res_A and d_last, z^ += corr, the restart pair applied to d_last + corr, the remaining terms - 1 steps"""
    pre = pn.pairs_of(coef, 0, terms)
    d, z, res = level.start(rhat, pre[0])
    for k in range(1, terms):
        d, z, res = level.step(d, z, res, pre[k][0], pre[k][1])
    rc = restrict(res) - (R @ d).astype(restrict(res).dtype)
    corr = prolong(coarse_solve(rc)).astype(level.dtype)
    z = z + corr
    d, z, res = level.step(d + corr, z, res, coef[o_restart], coef[o_restart + 1])
    for k in range(1, terms):
        d, z, res = level.step(d, z, res, pre[k][0], pre[k][1])
    return z


def two_level_cycle(fine, coarse, P, state, store_r=32):
    """pn.two_level_cycle with the restriction through R (first-kind smoother only)"""
    coef, ks = np.asarray(state["coef"], dtype=np.float64), state["ks"]
    restrict, prolong = pn._transfer(fine, coarse, P)
    cpairs = pn.pairs_of(coef, state["cf_coarse"], state["kc"])
    R = restricted_operator(fine, coarse, P, store_r)

    def apply(r):
        r = np.asarray(r, dtype=np.float64)
        zh = _merged_cycle_hat(fine, (fine.sc * r).astype(fine.dtype), coef, ks, state["cf_restart"], R, restrict,
                               lambda rc: coarse.poly_hat(rc, cpairs), prolong)
        return fine.sc * zh.astype(np.float64)
    return apply


def three_level_cycle(fine, mid, lvl3, P, P2, state, store_r=32):
    """pn.three_level_cycle with the FINE restriction through R; the vertex level keeps its own residual pass"""
    coef, ks, ks2 = np.asarray(state["coef"], dtype=np.float64), state["ks"], state["ks2"]
    o_c, o3 = state["cf_coarse"], state["cf_level3"]
    r12, p12 = pn._transfer(fine, mid, P)
    r23, p23 = pn._transfer(mid, lvl3, P2)
    pairs3 = pn.pairs_of(coef, o3, state["k3"])
    ones = np.ones(max(ks2, 1))
    R = restricted_operator(fine, mid, P, store_r)

    def corr3(res2):
        return p23(lvl3.poly_hat(r23(res2), pairs3))

    def mid_solve(rc):
        return pn._smoothed_cycle_hat(mid, rc, coef, o_c, ks2, o_c + 2 * ks2, o_c + 2 * ks2 + 2, ones, corr3)

    def apply(r):
        r = np.asarray(r, dtype=np.float64)
        zh = _merged_cycle_hat(fine, (fine.sc * r).astype(fine.dtype), coef, ks, state["cf_restart"], R, r12, mid_solve, p12)
        return fine.sc * zh.astype(np.float64)
    return apply


def operator_from(data, state, dtype=np.float64, store_r=32):
    """pn.operator_from for the p-multigrid configurations, with the merged fine level"""
    assert state["precond"] == 2 and state["smoother"] == 1
    store = int(data["store"])
    H, Hc = pn.unpack_csr("H", data), pn.unpack_csr("Hc", data)
    fine, mid = pn.Level(H, store, dtype), pn.Level(Hc, store, dtype)
    P = pn.prolongation_p(data["par0"], data["par1"], Hc.shape[0] // 3)
    if state["levels"] == 2:
        return two_level_cycle(fine, mid, P, state, store_r)
    H3 = pn.unpack_csr("H3", data)
    P2 = pn.prolongation_rbm(data["agg"], data["rvec"], H3.shape[0] // 6)
    return three_level_cycle(fine, mid, pn.Level(H3, store, dtype), P, P2, state, store_r)


def restricted_operator_blocks(f_off, f_cols, f_vals, sc_f, sc_c, par0, par1):
    """R from its definition, block by block in fp64, from the fine copy AS STORED (node-block CSR f_off / f_cols /
    f_vals [blocks, 3, 3]):  R[I,j]_de = sc_c[I,d] sum_i w_i Hs[i,j]_de / sc_f[i,d].  Returns (off, cols, vals, mag) with
    mag = sc_c[I,d] sum_i |w_i Hs[i,j]_de / sc_f[i,d]|, the size of the terms of every entry."""
    N, Nc = len(f_off) - 1, len(sc_c) // 3
    rows = np.repeat(np.arange(N), np.diff(f_off))
    scf, scc = np.asarray(sc_f).reshape(-1, 3), np.asarray(sc_c).reshape(-1, 3)
    scaled = f_vals / scf[rows][:, :, None]
    key_I, key_j, terms = [], [], []
    for which, par in enumerate((par0, par1)):
        par = np.asarray(par)
        use = (par[rows] >= 0) if which == 0 else ((par[rows] >= 0) & (np.asarray(par0)[rows] != par[rows]))
        w = np.where(np.asarray(par0)[rows] == np.asarray(par1)[rows], 1.0, 0.5)
        key_I.append(par[rows][use]); key_j.append(np.asarray(f_cols)[use]); terms.append((w[:, None, None] * scaled)[use])
    I, j, t = np.concatenate(key_I), np.concatenate(key_j), np.concatenate(terms)
    order = np.lexsort((j, I))
    I, j, t = I[order], j[order], t[order]
    first = np.concatenate([[True], (I[1:] != I[:-1]) | (j[1:] != j[:-1])])
    grp = np.cumsum(first) - 1
    nb = int(grp[-1]) + 1
    vals, mags = np.zeros((nb, 3, 3)), np.zeros((nb, 3, 3))
    np.add.at(vals, grp, t)
    np.add.at(mags, grp, np.abs(t))
    bI, bj = I[first], j[first]
    vals *= scc[bI][:, :, None]
    mags *= scc[bI][:, :, None]
    off = np.zeros(Nc + 1, dtype=np.int64)
    np.add.at(off, bI + 1, 1)
    return np.cumsum(off), bj, vals, mags
