"""The CG preconditioner M^-1 of the Newton solver restated in plain numpy / scipy ("Linear solve": the
polynomial, the p-multigrid cycles, the ANCF node-block form), written from the sequence of linear maps DESIGN and the
comments of cheb_apply / pmg_apply state -- not from the kernels.  tests/test_precond_np.py checks this file against mathematics,
tests/precond_worker.py compares the device with it vector by vector.

Every level is a `Level`: the symmetrically scaled matrix Hs = S H S (S = diag(H)^-1/2 per DOF, 1 where the diagonal is
not positive) with its entries rounded through the storage type of the device's copy (store = 16, 32, or 64 = exact),
and the inverse 3 x 3 diagonal blocks (S D S)^-1, rounded to float32 where the device keeps them in float32 (store != 64).
A polynomial step in the scaled space is

    res^ -= Hs d ;  d' = c1 d + c2 (S D S)^-1 res^ ;  z^ += w d'

started from d = (S D S)^-1 res^ c2_0, z^ = w_0 d, res^ = S r, with the pairs (c1, c2) of the uploaded coefficient table
(GetPreconditionerState()["coef"]).  The weights w are 1 for the first-kind Chebyshev smoother.  The fourth-kind smoothers
(TLFEA_PMG_SMOOTHER = 3 / 4) differ in the table's pairs and weights (fourth_kind_pairs) and in one step: with weights
other than 1 the recurrence carries the residual of the unweighted iterate, so the cycle forms res^ = S r - Hs z^ anew
before it restricts.

`dtype` carries the work vectors (and the arithmetic on them) in float32 instead of float64: the distance between the
two is the fp32 arithmetic floor of an operator, with identical matrix rounding in both."""
import numpy as np
import scipy.sparse as sp


def node_csr_to_dof(off, cols, vals, n_nodes):
    """the engine's node-block layout [row][d][k][e] (RetrievePmgLevel, RetrievePmgLevel3) -> scipy CSR over DOFs"""
    off = np.asarray(off, dtype=np.int64)
    ro = np.zeros(3 * n_nodes + 1, dtype=np.int64)
    ci, va = [], []
    for I in range(n_nodes):
        deg = off[I + 1] - off[I]
        blk = vals[9 * off[I]:9 * off[I + 1]].reshape(3, deg, 3)
        cc = (3 * np.asarray(cols[off[I]:off[I + 1]], dtype=np.int64)[:, None] + np.arange(3)[None, :]).reshape(-1)
        for dd in range(3):
            ci.append(cc)
            va.append(blk[dd].reshape(-1))
            ro[3 * I + dd + 1] = ro[3 * I + dd] + 3 * deg
    return sp.csr_matrix((np.concatenate(va), np.concatenate(ci), ro), shape=(3 * n_nodes, 3 * n_nodes))


def round_store(a, store):
    """values as the device's copy holds them: through float16, float32, or exact (64)"""
    if store == 16:
        return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)
    if store == 32:
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    assert store == 64
    return np.asarray(a, dtype=np.float64)


def diag_blocks(H):
    """[n/3, 3, 3] diagonal blocks of a DOF-level sparse matrix"""
    n = H.shape[0] // 3
    H = sp.csr_matrix(H)
    D = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(3):
            D[:, a, b] = np.asarray(H[np.arange(n) * 3 + a, np.arange(n) * 3 + b]).reshape(-1)
    return D


class Level:
    """one level's scaled copy: sc, Hs = round(S H S), Dinv = round32((S D S)^-1), work dtype"""

    def __init__(self, H, store=64, dtype=np.float64):
        H = sp.csr_matrix(H, dtype=np.float64)
        H.sort_indices()
        n = H.shape[0]
        dg = H.diagonal()
        self.sc = np.where(dg > 0.0, 1.0 / np.sqrt(np.where(dg > 0.0, dg, 1.0)), 1.0)
        S = sp.diags(self.sc)
        Hs = (S @ H @ S).tocsr()
        Hs.data = round_store(Hs.data, store)
        D = diag_blocks(H)                                           # fp64 blocks of H; (S D S)^-1 from them
        s3 = self.sc.reshape(-1, 3)
        Dinv = np.linalg.inv(D * s3[:, :, None] * s3[:, None, :])
        if store != 64:
            Dinv = Dinv.astype(np.float32).astype(np.float64)
        self.n, self.dtype = n, dtype
        self.Hs = Hs.astype(dtype)
        self.Dinv = Dinv.astype(dtype)

    @classmethod
    def raw(cls, Hs, sc, Dinv, dtype=np.float64):
        """a level from an already transformed matrix (the node-block form)"""
        L = cls.__new__(cls)
        L.n, L.dtype, L.sc = Hs.shape[0], dtype, np.asarray(sc, dtype=np.float64)
        L.Hs, L.Dinv = sp.csr_matrix(Hs).astype(dtype), np.asarray(Dinv).astype(dtype)
        return L

    def dinv(self, v):
        return np.einsum("nij,nj->ni", self.Dinv, v.reshape(-1, 3)).reshape(-1)

    def start(self, rhat, pair):
        """d = (SDS)^-1 res^ c2_0 ; z^ = w0 d ; res^ = rhat.  pair = table[0:2] = (1/theta, w0 or 0 for 1)"""
        t = self.dtype
        rhat = np.asarray(rhat, dtype=t)
        d = self.dinv(rhat) * t(pair[0])
        w0 = t(pair[1]) if pair[1] != 0.0 else t(1.0)
        return d, w0 * d, rhat

    def step(self, d, z, res, c1, c2, w=1.0):
        t = self.dtype
        res = res - self.Hs @ d
        d = t(c1) * d + t(c2) * self.dinv(res)
        return d, z + t(w) * d, res

    def poly_hat(self, rhat, pairs):
        """the polynomial of `pairs` ([(1/theta, .), (c1, c2), ...]) in the scaled space: z^ from res^"""
        d, z, res = self.start(rhat, pairs[0])
        for c1, c2 in pairs[1:]:
            d, z, res = self.step(d, z, res, c1, c2)
        return z


def pairs_of(coef, start, count):
    c = np.asarray(coef, dtype=np.float64)
    return [(c[start + 2 * k], c[start + 2 * k + 1]) for k in range(count)]


def chebyshev_pairs(lam_hi, kappa, terms):
    """pairs of the Chebyshev iteration on [lam_hi / kappa, lam_hi] (Saad, Iterative Methods, Alg. 12.1): (1/theta, 0),
    then (rho_k rho_{k-1}, 2 rho_k / delta) -- for tables built on the CPU (the device's come from its own hook)"""
    b, a = lam_hi, lam_hi / kappa
    theta, delta = 0.5 * (b + a), 0.5 * (b - a)
    sigma = theta / delta
    rho = 1.0 / sigma
    out = [(1.0 / theta, 0.0)]
    for _ in range(1, terms):
        rho_new = 1.0 / (2.0 * sigma - rho)
        out.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return out


LOTTES_BETA = {1: [1.12500000000000], 2: [1.02387287570313, 1.26408905371085],
               3: [1.00842544782028, 1.08867839208730, 1.33753125909618],
               4: [1.00391310427285, 1.04035811188593, 1.14863498546254, 1.38268869241000]}


def fourth_kind_pairs(lam_hi, terms, optimised=True):
    """fourth-kind Chebyshev smoother (Lottes 2022, "Optimal polynomial smoothers for multigrid V-cycles"): d0 = 4/(3 rho)
    D^-1 r ; d_k = (2k-1)/(2k+3) d_{k-1} + (8k+4)/((2k+3) rho) D^-1 r_k ; z_k = z_{k-1} + beta_k d_{k-1}.
    Returns (pairs, weights); the first pair carries beta_1 where the first-kind table has 0."""
    betas = LOTTES_BETA[terms] if optimised else [1.0] * terms
    pairs = [(4.0 / (3.0 * lam_hi), betas[0])]
    pairs += [((2.0 * k - 1.0) / (2.0 * k + 3.0), (8.0 * k + 4.0) / ((2.0 * k + 3.0) * lam_hi)) for k in range(1, terms)]
    return pairs, betas


def cycle_state(fine_pairs, mid_pairs, level3_pairs=None, max_terms=12, betas=None):
    """a coefficient table in the cycle's layout from per-level pairs (first-kind smoothers): [fine smoother | (0, 0) |
    (0, 1/theta) | max_terms weights | vertex level | level 3].  Two levels: mid_pairs is the vertex-level polynomial.
    Three levels: mid_pairs is the vertex-level smoother, followed by its own residual and restart pairs."""
    ks = len(fine_pairs)
    coef = [v for p in fine_pairs for v in p] + [0.0, 0.0, 0.0, fine_pairs[0][0]] + [1.0] * max_terms
    if betas is not None:
        coef[2 * ks + 4:2 * ks + 4 + ks] = list(betas)
    st = dict(ks=ks, cf_resid=2 * ks, cf_restart=2 * ks + 2, cf_beta=2 * ks + 4, cf_coarse=2 * ks + 4 + max_terms,
              cf_level3=0, ks2=0, kc=0, k3=0)
    coef += [v for p in mid_pairs for v in p]
    if level3_pairs is None:
        st["kc"] = len(mid_pairs)
    else:
        st["ks2"] = len(mid_pairs)
        coef += [0.0, 0.0, 0.0, mid_pairs[0][0]]
        st["cf_level3"], st["k3"] = len(coef), len(level3_pairs)
        coef += [v for p in level3_pairs for v in p]
    st["coef"] = np.array(coef)
    return st


def lam_max_dinv_h(level):
    """largest eigenvalue of (S D S)^-1 Hs = that of D^-1 H, by dense eigenvalues (small test matrices only)"""
    Dinv = sp.block_diag(list(level.Dinv.astype(np.float64)), format="csr")
    return float(np.max(np.linalg.eigvals((Dinv @ level.Hs.astype(np.float64)).toarray()).real))


def polynomial(level, coef, degree):
    """z = p_deg(D^-1 H) D^-1 r from the first `degree` pairs of the table"""
    pairs = pairs_of(coef, 0, degree)

    def apply(r):
        r = np.asarray(r, dtype=np.float64)
        zh = level.poly_hat((level.sc * r).astype(level.dtype), pairs)
        return level.sc * zh.astype(np.float64)
    return apply


def prolongation_p(par0, par1, n_coarse):
    """P of the p-multigrid pair (fine T10 nodes <- vertex nodes): a vertex takes its coarse value, a mid-edge node the
    mean of its edge's two vertices; rows of nodes without a parent (par0 < 0) are zero.  DOF level (x) I3."""
    par0, par1 = np.asarray(par0, dtype=np.int64), np.asarray(par1, dtype=np.int64)
    has = np.where(par0 >= 0)[0]
    rows = np.concatenate([has, has])
    cols = np.concatenate([par0[has], par1[has]])
    Pn = sp.csr_matrix((np.full(2 * len(has), 0.5), (rows, cols)), shape=(len(par0), n_coarse))
    return sp.kron(Pn, sp.identity(3), format="csr")


def prolongation_rbm(agg, rvec, n_agg):
    """P2 of the third level (vertex nodes <- rigid-body modes of their aggregate): u_i = t_A + w_A x r_i, i.e. blocks
    W_i0 = I, W_i1 = -[r_i]x; r_i is zero where the aggregate's rotations are switched off"""
    rows, cols, vals = [], [], []
    for i, (A, r) in enumerate(zip(agg, rvec)):
        S = -np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        for a in range(3):
            rows.append(3 * i + a); cols.append(6 * A + a); vals.append(1.0)
            for b in range(3):
                if S[a, b] != 0.0:
                    rows.append(3 * i + a); cols.append(6 * A + 3 + b); vals.append(S[a, b])
    return sp.csr_matrix((vals, (rows, cols)), shape=(3 * len(agg), 6 * n_agg))


def level3_matrix(Hc, P2, active):
    """H3 = P2^T Hc P2 with identity rows for switched-off rotations (active 0) and empty aggregates (active < 0)"""
    H3 = sp.lil_matrix(P2.T @ sp.csr_matrix(Hc) @ P2)
    for A in np.where(np.asarray(active) <= 0)[0]:
        for c in range(3):
            H3[6 * A + 3 + c, 6 * A + 3 + c] = 1.0
    for A in np.where(np.asarray(active) < 0)[0]:
        for c in range(3):
            H3[6 * A + c, 6 * A + c] = 1.0
    return H3.tocsr()


def _smoothed_cycle_hat(level, rhat, coef, o_tab, terms, o_resid, o_restart, betas, coarse):
    """One level of a V-cycle in the scaled space: `terms` pre-smoothing terms, the residual, the coarse correction
    coarse(res^) -> corr^ (already in this level's scaled space), the restart pair (0, 1/theta) and the remaining
    terms - 1 steps.  Returns z^."""
    pre = pairs_of(coef, o_tab, terms)
    d, z, res = level.start(rhat, pre[0])
    for k in range(1, terms):
        d, z, res = level.step(d, z, res, pre[k][0], pre[k][1], betas[k])
    if np.all(np.asarray(betas[:terms]) == 1.0):
        d, z, res = level.step(d, z, res, coef[o_resid], coef[o_resid + 1])      # (0, 0): the residual of the result
    else:   # weighted updates: the recurrence carries the unweighted iterate's residual; the cycle needs that of z^
        res = level.start(rhat, pre[0])[2] - level.Hs @ z
    corr = coarse(res).astype(level.dtype)
    z = z + corr                                                                 # z^ += corr ; d := corr
    d, z, res = level.step(corr, z, res, coef[o_restart], coef[o_restart + 1], betas[0])
    for k in range(1, terms):
        d, z, res = level.step(d, z, res, pre[k][0], pre[k][1], betas[k])
    return z


def _transfer(fine, coarse, P):
    """restriction r^_c = S_c P^T S_f^-1 res^ and prolongation corr^ = S_f^-1 P S_c z^_c between two scaled spaces
    (fp64 arithmetic on the rounded work vectors, the results back in the work type)"""
    def restrict(res):
        return (coarse.sc * (P.T @ (res.astype(np.float64) / fine.sc))).astype(coarse.dtype)

    def prolong(zc):
        return ((P @ (coarse.sc * zc.astype(np.float64))) / fine.sc).astype(fine.dtype)
    return restrict, prolong


def two_level_cycle(fine, coarse, P, state, coarse_solve=None):
    """z = V-cycle(r): ks pre-smoothing terms, residual, r_c = P^T res, the coarse polynomial of degree kc, z += P e_c,
    the restart pair and the remaining ks - 1 terms.  state: GetPreconditionerState() (coef, ks, cf_*, kc).
    coarse_solve (tests): replaces the coarse polynomial, scaled residual -> scaled correction."""
    coef, ks = np.asarray(state["coef"], dtype=np.float64), state["ks"]
    betas = coef[state["cf_beta"]:state["cf_beta"] + max(ks, 1)]
    restrict, prolong = _transfer(fine, coarse, P)
    cpairs = pairs_of(coef, state["cf_coarse"], state["kc"]) if coarse_solve is None else None

    def coarse_corr(res):
        rc = restrict(res)
        zc = coarse.poly_hat(rc, cpairs) if coarse_solve is None else coarse_solve(rc)
        return prolong(zc)

    def apply(r):
        r = np.asarray(r, dtype=np.float64)
        zh = _smoothed_cycle_hat(fine, (fine.sc * r).astype(fine.dtype), coef, 0, ks, state["cf_resid"], state["cf_restart"],
                                 betas, coarse_corr)
        return fine.sc * zh.astype(np.float64)
    return apply


def three_level_cycle(fine, mid, lvl3, P, P2, state):
    """the same sequence with the vertex level as a smoothing level (ks2 terms, its table at cf_coarse: steps, residual
    pair, restart pair) around the level-3 polynomial of degree k3 (table at cf_level3)"""
    coef, ks, ks2 = np.asarray(state["coef"], dtype=np.float64), state["ks"], state["ks2"]
    betas = coef[state["cf_beta"]:state["cf_beta"] + max(ks, 1)]
    o_c, o3 = state["cf_coarse"], state["cf_level3"]
    r12, p12 = _transfer(fine, mid, P)
    r23, p23 = _transfer(mid, lvl3, P2)
    pairs3 = pairs_of(coef, o3, state["k3"])
    ones = np.ones(max(ks2, 1))

    def corr3(res2):
        return p23(lvl3.poly_hat(r23(res2), pairs3))

    def corr2(res):
        z2 = _smoothed_cycle_hat(mid, r12(res), coef, o_c, ks2, o_c + 2 * ks2, o_c + 2 * ks2 + 2, ones, corr3)
        return p12(z2)

    def apply(r):
        r = np.asarray(r, dtype=np.float64)
        zh = _smoothed_cycle_hat(fine, (fine.sc * r).astype(fine.dtype), coef, 0, ks, state["cf_resid"], state["cf_restart"],
                                 betas, corr2)
        return fine.sc * zh.astype(np.float64)
    return apply


def node_block_form(H, coef, degree, store=64, dtype=np.float64, linv32=True):
    """ANCF: z = L^-T p(L^-1 H L^-T) L^-1 r with the 12 x 12 node blocks D12 = L L^T (np.linalg.cholesky).  The streamed
    matrix L^-1 H L^-T comes from the fp64 L^-1 and is rounded through `store`; the two applications of L^-1 / L^-T use
    its float32 copy (linv32), as the device's do, in fp64 arithmetic.  Its own 3 x 3 scaling is the identity."""
    H = sp.csr_matrix(H, dtype=np.float64)
    n = H.shape[0]
    assert n % 12 == 0
    blocks = []
    for p in range(n // 12):
        D12 = H[12 * p:12 * p + 12, 12 * p:12 * p + 12].toarray()
        blocks.append(np.linalg.inv(np.linalg.cholesky(D12)))
    Linv = sp.block_diag(blocks, format="csr")
    Hh = (Linv @ H @ Linv.T).tocsr()
    Hh.data = round_store(Hh.data, store)
    Lf = sp.block_diag([b.astype(np.float32).astype(np.float64) for b in blocks], format="csr") if linv32 else Linv
    level = Level.raw(Hh, np.ones(n), np.broadcast_to(np.eye(3), (n // 3, 3, 3)).copy(), dtype)
    inner = polynomial(level, coef, degree)

    def apply(r):
        return Lf.T @ inner(Lf @ np.asarray(r, dtype=np.float64))
    apply.Linv, apply.Hhat = Linv, Hh
    return apply


def pack_csr(prefix, M):
    M = sp.csr_matrix(M)
    return {prefix + "_data": M.data, prefix + "_indices": M.indices, prefix + "_indptr": M.indptr,
            prefix + "_shape": np.array(M.shape)}


def unpack_csr(prefix, d):
    return sp.csr_matrix((d[prefix + "_data"], d[prefix + "_indices"], d[prefix + "_indptr"]), shape=tuple(d[prefix + "_shape"]))


LAYOUT_KEYS = ("precond", "levels", "degree", "ks", "cf_resid", "cf_restart", "cf_beta", "cf_coarse", "cf_level3", "ks2", "kc",
               "k3", "smoother", "block")


def layout_of(state):
    """the integers of GetPreconditionerState() a restatement needs, in the order of LAYOUT_KEYS"""
    return np.array([state[k] for k in LAYOUT_KEYS])


def pack_device_state(s, H, store, state, info):
    """what operator_from() needs from the device besides the coefficient table, as arrays an npz holds: H, the storage
    bits and, for the cycles, the parent map and the coarse operators of the solver s (shared by the workers of
    tests/test_gpu_precond_operator.py and tests/test_gpu_cg_trace.py).  Sizes of the coarse levels go into `info`."""
    data = dict(store=store, **pack_csr("H", H))
    if state["precond"] == 2:
        par0, par1, c_off, c_cols, Hc = s.RetrievePmgLevel()
        nc = len(c_off) - 1
        vb = np.diff(c_off)
        data.update(par0=par0, par1=par1, **pack_csr("Hc", node_csr_to_dof(c_off, c_cols, Hc, nc)))
        info.update(n_vertex=int(nc), vertex_blocks_max=int(vb.max()), vertex_blocks=int(vb.sum()))
        if state["levels"] == 3:
            agg, rvec, active, off3, cols3, H3 = s.RetrievePmgLevel3()
            na = len(active)
            data.update(agg=agg, rvec=rvec, **pack_csr("H3", node_csr_to_dof(off3, cols3, H3, 2 * na)))
            info.update(n_aggregates=int(na), inactive_rotations=int((active == 0).sum()), empty_cells=int((active < 0).sum()))
    return data


def operator_from(data, state, dtype=np.float64):
    """the restated M^-1 of a configuration: data holds H (pack_csr "H"), store, and for the cycles par0 / par1 and Hc
    ("Hc"), for three levels agg / rvec and H3 ("H3"); state is GetPreconditionerState() of the set-up to restate"""
    store = int(data["store"])
    H = unpack_csr("H", data)
    if state["precond"] == 1:
        if state["block"] == 12:
            return node_block_form(H, state["coef"], state["degree"], store, dtype)
        return polynomial(Level(H, store, dtype), state["coef"], state["degree"])
    assert state["precond"] == 2
    Hc = unpack_csr("Hc", data)
    fine, mid = Level(H, store, dtype), Level(Hc, store, dtype)
    P = prolongation_p(data["par0"], data["par1"], Hc.shape[0] // 3)
    if state["levels"] == 2:
        return two_level_cycle(fine, mid, P, state)
    H3 = unpack_csr("H3", data)
    P2 = prolongation_rbm(data["agg"], data["rvec"], H3.shape[0] // 6)
    return three_level_cycle(fine, mid, Level(H3, store, dtype), P, P2, state)


def dense_of(op, n):
    """the operator as a dense matrix: applied to the identity, column by column"""
    M = np.zeros((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        M[:, j] = op(e)
        e[j] = 0.0
    return M


def pcg(H, b, precond, rel_tol=1e-12, max_iter=20000):
    """plain preconditioned CG in fp64 from x = 0; stops at ||r|| <= rel_tol ||b|| tested after every iteration.
    Returns (x, iterations, ||r|| / ||b||)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    r = b.copy()
    bb = float(b @ b)
    if bb == 0.0:
        return x, 0, 0.0
    z = precond(r)
    p = z.copy()
    rz = float(r @ z)
    it = 0
    while it < max_iter:
        q = H @ p
        alpha = rz / float(p @ q)
        x += alpha * p
        r -= alpha * q
        it += 1
        if float(r @ r) <= rel_tol * rel_tol * bb:
            break
        z = precond(r)
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it, float(np.sqrt(float(r @ r) / bb))
