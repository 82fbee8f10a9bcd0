"""The V-cycle whose fine smoother applies H itself (DESIGN 3g'), restated next to tests/precond_np.py and
tests/restricted_op_np.py (both imported, neither edited).  The fine level holds the scaled operator Hs = S H S exactly
(nothing is rounded through fp16; the device forms Hs d element by element in float32) and the float32 (S D S)^-1 the
device keeps; R = S_c P^T S_f^-1 Hs = S_c P^T H S_f comes from that same operator, rounded once to float32; the vertex
level and the third level keep their fp16 copies.  ElementLevel forms Hs d the way the device does -- the element map of
tests/matfree_np.py in the work type, with the device's normalisation -- and the distance between float32 and float64 work
vectors through it is the fp32 arithmetic floor of a pass and of the operator.  fine_level / operator_from are the same
with Hs as a CSR matrix (what R is built from; a cross-check of the element map in float64)."""
import numpy as np

from tests import precond_np as pn
from tests import restricted_op_np as rn

COARSE_STORE = 16


def fine_level(H, dtype=np.float64):
    """the fine level on the exact operator: Hs unrounded, (S D S)^-1 through float32"""
    L = pn.Level(H, 64, dtype)
    L.Dinv = L.Dinv.astype(np.float32).astype(dtype)
    return L


def operator_from(data, state, dtype=np.float64):
    """rn.operator_from with the exact fine level"""
    assert state["precond"] == 2 and state["smoother"] == 1
    H, Hc = pn.unpack_csr("H", data), pn.unpack_csr("Hc", data)
    fine, mid = fine_level(H, dtype), pn.Level(Hc, COARSE_STORE, dtype)
    P = pn.prolongation_p(data["par0"], data["par1"], Hc.shape[0] // 3)
    if state["levels"] == 2:
        return rn.two_level_cycle(fine, mid, P, state, 32)
    H3 = pn.unpack_csr("H3", data)
    P2 = pn.prolongation_rbm(data["agg"], data["rvec"], H3.shape[0] // 6)
    return rn.three_level_cycle(fine, mid, pn.Level(H3, COARSE_STORE, dtype), P, P2, state, 32)


def scaled_blocks(H, f_off, f_cols, sc_f):
    """Hs = S H S block by block, [blocks, 3, 3] on the node pattern (f_off, f_cols), in fp64: what
    rn.restricted_operator_blocks takes where the stored copy stood"""
    H = H.tocsr()
    N = len(f_off) - 1
    rows = np.repeat(np.arange(N), np.diff(f_off))
    cols = np.asarray(f_cols, dtype=np.int64)
    out = np.zeros((len(cols), 3, 3))
    for d in range(3):
        for e in range(3):
            out[:, d, e] = np.asarray(H[3 * rows + d, 3 * cols + e]).reshape(-1)
    s = np.asarray(sc_f).reshape(-1, 3)
    return out * s[rows][:, :, None] * s[cols][:, None, :]


def symmetry_defect(op, n, seed=5):
    """|x.M y - y.M x| / (|x| |M y|) on two pairs of normal vectors, the figure of tests/precond_worker.py"""
    v = np.random.default_rng(seed).normal(size=(3, n))
    z = [op(x) for x in v]
    return max(abs(v[a] @ z[b] - v[b] @ z[a]) / (np.linalg.norm(v[a]) * np.linalg.norm(z[b])) for a, b in ((0, 1), (1, 2)))


# ---- the pass as the device forms it: the element map of tests/matfree_np.py in the work type -----------------------------
def element_problem(X, conn, x, quad, E, nu, rho0, h, eta, lamd, fixed, rho_pen):
    """what the element map needs, in fp64: the records (g, det J, F at the rule's points), the rule's tables, the scalars
    of the assembled H and the pinned nodes.  Arrays only, so that an npz holds it."""
    from tests import matfree_np as mf
    qx, qy, qz, qw = (np.asarray(a, dtype=np.float64) for a in quad)
    g, detJ = mf.vertex_gradients(np.asarray(X, dtype=np.float64), conn)
    Nq, c = mf.shape_tables(qx, qy, qz)
    gradN = np.einsum("qjn,end->eqjd", c, g)
    F = np.einsum("eji,eqjd->eqid", np.asarray(x, dtype=np.float64)[conn], gradN)
    lam, mu = (E * nu) / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))
    return dict(ep_conn=np.asarray(conn, dtype=np.int64), ep_g=g, ep_detJ=detJ, ep_F=F, ep_Nq=Nq, ep_c=c, ep_qw=qw,
                ep_fixed=np.asarray(fixed, dtype=np.int64),
                ep_scal=np.array([h * lam + lamd, h * mu + eta, h * mu, h * lam, rho0 / h, h * h * rho_pen]))


class ElementLevel(pn.Level):
    """fine_level whose product Hs d is formed element by element in the work type, as the device's pair forms it: float
    copies of the fp64 records, the material scalars divided by m0 = max(|a|, |b|, |c1|, |cl|), the direction
    x = scn d with scn = (sc / sigma) in the work type, sigma^2 = mean(sc^2), the node sums (+ the pinned-row term) times
    tau scn, tau = m0 sigma^2.  In float64 this is Hs d itself."""

    def __init__(self, H, ep, dtype=np.float64):
        base = fine_level(H, dtype)
        self.__dict__.update(base.__dict__)
        t = dtype
        a, b, c1, cl, rho_h, pen = (float(v) for v in ep["ep_scal"])
        m0 = max(abs(a), abs(b), abs(c1), abs(cl))
        sig2 = float(np.mean(self.sc ** 2))
        self.scn = (self.sc / np.sqrt(sig2)).astype(t)
        self.tau = t(m0 * sig2)
        self.k = [t(v / m0) for v in (a, b, c1, cl, rho_h)]
        self.pen = t(pen / m0)
        self.conn, self.fixed = ep["ep_conn"], ep["ep_fixed"]
        self.g, self.detJ, self.F = ep["ep_g"].astype(t), ep["ep_detJ"].astype(t), ep["ep_F"].astype(t)
        self.Nq, self.c, self.qw = ep["ep_Nq"].astype(t), ep["ep_c"].astype(t), ep["ep_qw"].astype(t)
        # what does not depend on the direction, once (in the work type, as every pass would form it)
        a, b, c1, cl, rho_h = self.k
        I = np.eye(3, dtype=t)
        self.gradN = np.einsum("qjn,end->eqjd", self.c, self.g)
        C = np.einsum("eqki,eqkj->eqij", self.F, self.F)
        trE = t(0.5) * (np.trace(C, axis1=2, axis2=3) - t(3))
        self.Sh = (cl * trE - c1)[..., None, None] * I + c1 * C           # h (lambda tr E I + 2 mu E) / m0
        self.dV = self.detJ[:, None] * self.qw[None, :]
        assert self.gradN.dtype == t and self.Sh.dtype == t and self.dV.dtype == t

    def hs(self, d):
        t = self.dtype
        a, b, c1, cl, rho_h = self.k
        x = self.scn * np.asarray(d, dtype=t)
        pe = x.reshape(-1, 3)[self.conn]
        gradN, F, Sh, dV = self.gradN, self.F, self.Sh, self.dV
        dF = np.einsum("eji,eqjd->eqid", pe, gradN)
        I = np.eye(3, dtype=t)
        G = np.einsum("eqki,eqkj->eqij", F, dF)
        dS = (a * np.trace(G, axis1=2, axis2=3))[..., None, None] * I + b * (G + G.transpose(0, 1, 3, 2))
        dP = np.einsum("eqik,eqkj->eqij", dF, Sh) + np.einsum("eqik,eqkj->eqij", F, dS)
        ye = np.einsum("eq,eqid,eqjd->eji", dV, dP, gradN)
        ye = ye + rho_h * np.einsum("eq,qi,qj,ejd->eid", dV, self.Nq, self.Nq, pe)
        assert ye.dtype == t
        y = np.zeros((self.n // 3, 3), dtype=t)
        np.add.at(y, self.conn, ye)
        y = y.reshape(-1)
        if len(self.fixed):
            dof = (3 * self.fixed[:, None] + np.arange(3)[None, :]).reshape(-1)
            y[dof] += self.pen * x[dof]
        return self.tau * self.scn * y

    def step(self, d, z, res, c1, c2, w=1.0):
        t = self.dtype
        res = res - self.hs(d)
        d = t(c1) * d + t(c2) * self.dinv(res)
        return d, z + t(w) * d, res


def last_pass(level, d, z, res, r, c1, c2, w=1.0):
    """the last pass: a step, then z = S z^ in fp64 and r.z"""
    d, z, res = level.step(d, z, res, c1, c2, w)
    z64 = level.sc * z.astype(np.float64)
    return d, z64, float(np.asarray(r, dtype=np.float64) @ z64)


def element_operator_from(data, state, dtype=np.float64):
    """operator_from with the fine passes formed element by element (ElementLevel); R from the exact operator"""
    assert state["precond"] == 2 and state["smoother"] == 1
    H, Hc = pn.unpack_csr("H", data), pn.unpack_csr("Hc", data)
    fine, mid = ElementLevel(H, data, dtype), pn.Level(Hc, COARSE_STORE, dtype)
    P = pn.prolongation_p(data["par0"], data["par1"], Hc.shape[0] // 3)
    coef, ks = np.asarray(state["coef"], dtype=np.float64), state["ks"]
    restrict, prolong = pn._transfer(fine, mid, P)
    R = rn.restricted_operator(fine_level(H, dtype), mid, P, 32)
    if state["levels"] == 2:
        cpairs = pn.pairs_of(coef, state["cf_coarse"], state["kc"])

        def mid_solve(rc):
            return mid.poly_hat(rc, cpairs)
    else:
        H3 = pn.unpack_csr("H3", data)
        P2 = pn.prolongation_rbm(data["agg"], data["rvec"], H3.shape[0] // 6)
        lvl3 = pn.Level(H3, COARSE_STORE, dtype)
        r23, p23 = pn._transfer(mid, lvl3, P2)
        pairs3 = pn.pairs_of(coef, state["cf_level3"], state["k3"])
        o_c, ks2 = state["cf_coarse"], state["ks2"]
        ones = np.ones(max(ks2, 1))

        def mid_solve(rc):
            return pn._smoothed_cycle_hat(mid, rc, coef, o_c, ks2, o_c + 2 * ks2, o_c + 2 * ks2 + 2, ones,
                                          lambda res2: p23(lvl3.poly_hat(r23(res2), pairs3)))

    def apply(r):
        r = np.asarray(r, dtype=np.float64)
        zh = rn._merged_cycle_hat(fine, (fine.sc * r).astype(fine.dtype), coef, ks, state["cf_restart"], R, restrict, mid_solve,
                                  prolong)
        return fine.sc * zh.astype(np.float64)
    return apply
