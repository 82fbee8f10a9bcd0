"""The numpy restatement of the adjoint step (tests/adjoint_np.py) against central differences of the CPU oracle's
implicit step on the cube mesh: fixed nodes, max_outer = 1, random f_ext, v_prev, perturbed x_prev, nonzero lambda and a
body acceleration (the oracle has none: f_ext + M a is the same load).  Every output, SVK and Mooney-Rivlin.

Bound: 1e-5 relative per directional derivative.  The central difference of a step solved to ||g|| < inner_atol carries
(solve error) / (step) + O(step^2): with the steps below both stay orders of magnitude under the bound."""
import numpy as np
import pytest

from oracle import orc
from tests import adjoint_np as anp
from tests.helpers import MATERIALS, fixed_x0, load_mesh

H_STEP, RHO = 1e-3, 1e10
ATOL = 1e-5   # on ||g||, whose terms are of the order 1e4: the Newton loop stops at the rounding floor of g
BOUND = 1e-5


class Problem:
    def __init__(self, kind, seed=7):
        self.X, self.conn = load_mesh("cube")
        self.N = self.X.shape[0]
        self.fixed = fixed_x0(self.X)
        assert 0 < len(self.fixed) < self.N
        rng = np.random.default_rng(seed)
        self.m = dict(MATERIALS[kind])
        self.kind = kind
        svk = orc.svk(self.m.get("E", 1.0), self.m.get("nu", 0.0))
        self.theta = (np.array([self.m["mu10"], self.m["mu01"], self.m["kappa"]]) if kind == "mr" else
                      np.array([svk.lam, svk.mu]))
        self.rho0 = self.m["rho0"]
        n, nc = 3 * self.N, 3 * len(self.fixed)
        L = np.ptp(self.X, axis=0).max()
        self.x_prev = self.X + rng.normal(0.0, 2e-3 * L, self.X.shape)
        self.v_prev = rng.normal(0.0, 0.2, n)
        self.lam = rng.normal(0.0, 1e3, nc)
        self.f_ext = rng.normal(0.0, 1e4, n)
        self.a = np.array([0.3, -9.81, 2.0])
        self.targets = self.X[self.fixed] + rng.normal(0.0, 1e-4 * L, (len(self.fixed), 3))
        # cotangents of x, v, lambda_new: lambda_new moves by rho per unit of x, so its weights are scaled by 1 / rho to
        # keep the three contributions to the right-hand side comparable
        self.xbar, self.vbar = rng.normal(0.0, 1.0, n), rng.normal(0.0, H_STEP, n)
        self.lambar = rng.normal(0.0, 1.0 / RHO, nc)

    def material(self, theta, rho0):
        if self.kind == "mr":
            return orc.mooney_rivlin(theta[0], theta[1], theta[2], rho0=rho0)
        return orc.svk_lame(theta[0], theta[1], rho0=rho0)

    def step(self, x_prev=None, v_prev=None, lam=None, f_ext=None, a=None, targets=None, theta=None, rho0=None):
        """one implicit step of the oracle -> (oracle at the converged state, x [3N], v, lam_new)"""
        pick = lambda v, d: d if v is None else v  # noqa: E731
        x_prev, v_prev, lam = pick(x_prev, self.x_prev), pick(v_prev, self.v_prev), pick(lam, self.lam)
        f_ext, a, targets = pick(f_ext, self.f_ext), pick(a, self.a), pick(targets, self.targets)
        theta, rho0 = pick(theta, self.theta), pick(rho0, self.rho0)
        o = orc.T10Oracle(self.X, self.conn, self.material(theta, rho0), fixed=self.fixed)
        o.calc_dndu_pre()
        o.calc_mass()
        o.f_ext = f_ext + anp.mass_times(o.m_off, o.m_col, o.m_val, np.tile(a, self.N))
        o.x, o.y, o.z = (np.ascontiguousarray(x_prev[:, i]).copy() for i in range(3))
        o.xt[self.fixed], o.yt[self.fixed], o.zt[self.fixed] = targets[:, 0], targets[:, 1], targets[:, 2]
        o.v, o.v_prev, o.lam = v_prev.copy(), v_prev.copy(), lam.copy()
        st = o.newton_step(orc.NewtonParams(ATOL, 0.0, 1e-6, RHO, 1, 30, H_STEP), solver=0)
        assert st[2] < ATOL, f"the oracle's step did not converge: ||g|| = {st[2]:.3e}"
        return o, np.stack([o.x, o.y, o.z], axis=1).reshape(-1), o.v.copy(), o.lam.copy()

    def loss(self, **kw):
        _, x, v, lam = self.step(**kw)
        return self.xbar @ x + self.vbar @ v + self.lambar @ lam

    def central(self, name, direction, eps):
        base = getattr(self, name)
        d = np.asarray(direction, dtype=np.float64).reshape(np.shape(base))
        return (self.loss(**{name: base + eps * d}) - self.loss(**{name: base - eps * d})) / (2.0 * eps)


@pytest.fixture(scope="module", params=["svk", "mr"])
def case(request):
    """the converged step, its restated adjoint and the central differences of every input, computed once per model"""
    p = Problem(request.param)
    o, x, v, lam_new = p.step()
    ro, ci, val = o.assemble_hessian(H_STEP, RHO)
    n = 3 * p.N
    H = np.zeros((n, n))
    for r in range(n):
        H[r, ci[ro[r]:ro[r + 1]]] += val[ro[r]:ro[r + 1]]
    H = np.triu(H) + np.triu(H, 1).T if np.allclose(np.tril(H, -1), 0.0) else H
    J = anp.selector_J(p.fixed, p.N)
    X1 = x.reshape(-1, 3)
    gradN = o.gradN_a_d()
    F = anp.deformation_gradients(X1, p.conn, gradN)
    Nq = anp.shape_values(o.qx, o.qy, o.qz)
    u = (v - p.v_prev) / H_STEP - np.tile(p.a, p.N)
    rng = np.random.default_rng(11)
    dirs = dict(f_ext=rng.normal(size=n), v_prev=rng.normal(size=n), x_prev=rng.normal(size=(p.N, 3)),
                lam=rng.normal(size=len(p.lam)), targets=rng.normal(size=p.targets.shape))
    # relative steps: 1e-4 of the moduli, 1e-3 of the density; the vectors move by 1e-4 of their own scale
    scale = dict(f_ext=1e4, v_prev=0.2, x_prev=2e-3, lam=1e3, targets=1e-4)
    fd = {k: p.central(k, d, 1e-2 * scale[k] / np.abs(d).max()) for k, d in dirs.items()}
    fd["gravity"] = np.array([p.central("a", np.eye(3)[c], 1e-3 * 9.81) for c in range(3)])
    fd["theta"] = np.array([p.central("theta", np.eye(len(p.theta))[k], 1e-4 * p.theta[k]) for k in range(len(p.theta))])
    fd["rho0"] = p.central("rho0", 1.0, 1e-3 * p.rho0)

    def restated(**kw):
        w, out = anp.adjoint_step(H, o.m_off, o.m_col, o.m_val, J, H_STEP, RHO, p.xbar, p.vbar, p.lambar, **kw)
        pe = anp.sens_per_element(F, gradN, o.detJ, o.qw, p.conn, w, u, "mr" if p.kind == "mr" else "svk", Nq)
        got = {k: float(np.dot(out[k].reshape(-1), np.asarray(d).reshape(-1))) for k, d in dirs.items()
               if k not in ("lam",)}
        got["lam"] = float(out["lam_in"] @ dirs["lam"])
        got["gravity"] = out["gravity"]
        pm = anp.per_material(pe, None, 1)[0]
        got["theta"], got["rho0"] = pm[:-1], pm[-1]
        return w, pe, got
    w, pe, got = restated()
    return dict(p=p, o=o, w=w, pe=pe, got=got, fd=fd, restated=restated, x=x)


def gaps(got, fd):
    out = {}
    for k, ref in fd.items():
        g, r = np.atleast_1d(got[k]).astype(float), np.atleast_1d(ref).astype(float)
        for i in range(len(r)):
            out[f"{k}[{i}]" if len(r) > 1 else k] = abs(g[i] - r[i]) / abs(r[i])
    return out


def test_every_output_matches_central_differences(case):
    g = gaps(case["got"], case["fd"])
    for k, v in g.items():
        print(f"{case['p'].kind} {k}: relative gap {v:.3e}")
    bad = {k: v for k, v in g.items() if not v <= BOUND}
    assert not bad, f"adjoint restatement differs from central differences beyond {BOUND}: {bad}"


def test_stiffness_slots_through_the_oracle(case):
    """-w . f_int with unit moduli is the same number by linearity of P in its parameters"""
    p, o, w = case["p"], case["o"], case["w"]
    for k in range(len(p.theta)):
        unit = np.zeros(len(p.theta))
        unit[k] = 1.0
        o.mat = p.material(unit, p.rho0)
        via_oracle = -float(w @ o.internal_force())
        direct = case["got"]["theta"][k]
        terms = float(np.abs(case["pe"][:, k]).sum())
        assert abs(via_oracle - direct) <= 1e-10 * terms, (k, via_oracle, direct)
        assert abs(via_oracle - case["fd"]["theta"][k]) <= BOUND * abs(case["fd"]["theta"][k])
    o.mat = p.material(p.theta, p.rho0)


def test_material_sums_do_not_depend_on_the_order(case):
    """the bound the GPU's per-material sums are held to (1e-12 sum |s_e|) covers fp64 sums in any order"""
    pe = case["pe"]
    fwd = pe.sum(axis=0)
    rev = pe[::-1].sum(axis=0)
    seq = np.zeros(pe.shape[1])
    for row in pe[np.random.default_rng(3).permutation(len(pe))]:
        seq = seq + row
    tol = 1e-12 * np.abs(pe).sum(axis=0)
    assert np.all(np.abs(fwd - rev) <= tol) and np.all(np.abs(fwd - seq) <= tol)


@pytest.mark.parametrize("mistake", [dict(sign=-1.0), dict(drop_jt=True)])
def test_the_check_catches_a_wrong_restatement(case, mistake):
    """a flipped sign of w, or x_t without rho J^T lambar, must miss the bound"""
    _, _, wrong = case["restated"](**mistake)
    g = gaps(wrong, case["fd"])
    assert max(g.values()) > 100 * BOUND, g
    if "drop_jt" in mistake:  # every output that reads w is off, not only one
        assert sum(v > BOUND for v in g.values()) >= len(g) // 2, g
