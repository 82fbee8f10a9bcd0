"""The numpy restatement of the ANCF adjoint step (tests/ancf_adjoint_np.py) against central differences of the CPU
oracle's implicit step: AncfOracle.newton_step (fixed coefficients) on five beams and on the 2 x 2 shell plate, and
AncfOracle.newton_step_lin (CSR rows) on the five beams; max_outer = 1, random f_ext, v_prev, perturbed x_prev, nonzero
lambda and a body acceleration on the position coefficients (the oracle has none: f_ext + M a^ is the same load).  Every
output, SVK and Mooney-Rivlin.

Bound: 1e-5 of the output's largest component, as tests/test_adjoint_np.py.  The steps of the central differences come
from a halving study (STEP below); test_difference_steps_sit_on_the_plateau halves them again on the thin shell and finds
every gap still orders of magnitude under the bound.  Measured largest gap per case: beam5 fixed 1.6e-8 (SVK) / 1.1e-7
(MR), plate2x2 2.9e-8 / 4.3e-8, beam5 with CSR rows 4.6e-7 / 1.8e-6."""
import functools

import numpy as np
import pytest

from oracle import orc
from tests import adjoint_np as tnp
from tests import ancf_adjoint_np as aad
from tests import ancf_stress_np as anp
from tests.helpers import MATERIALS

H_STEP, RHO = 1e-3, 1e10
ATOL = 1e-5   # on ||g||, whose terms are of the order 1e4: the Newton loop stops at the rounding floor of g
BOUND = 1e-5
SHAPES = {"beam5": lambda: anp.beam_line(5), "plate2x2": lambda: anp.shell_plate(2, 2)}
CASES = [("beam5", "fixed"), ("plate2x2", "fixed"), ("beam5", "csr")]


def clamped_coefficients(x12):
    """all four coefficient vectors of the mesh nodes on the plane x = 0"""
    nodes = np.where(np.abs(np.asarray(x12)[0::4]) < 1e-12)[0]
    return np.concatenate([4 * n + np.arange(4) for n in nodes]).astype(np.int32)


def csr_rows(fixed, X, n_coef):
    """the clamped coefficients pinned component by component, and the z of the last two nodes' positions tied"""
    rows, rhs = [], []
    for c in fixed:
        for k in range(3):
            rows.append(([3 * c + k], [1.0]))
            rhs.append(X[c, k])
    a, b = n_coef - 4, n_coef - 8
    rows.append(([3 * a + 2, 3 * b + 2], [1.0, -1.0]))
    rhs.append(X[a, 2] - X[b, 2])
    off = np.cumsum([0] + [len(r[0]) for r in rows]).astype(np.int32)
    return off, np.concatenate([r[0] for r in rows]).astype(np.int32), np.concatenate([r[1] for r in rows]), np.array(rhs)


class Problem:
    def __init__(self, shape, cons, kind, seed=7):
        self.prob = SHAPES[shape]()
        self.shape, self.cons, self.kind = shape, cons, kind
        self.X = np.stack(self.prob[1:4], axis=1)
        self.N = self.X.shape[0]
        self.fixed = clamped_coefficients(self.prob[1])
        assert 0 < len(self.fixed) < self.N
        rng = np.random.default_rng(seed)
        self.m = dict(MATERIALS[kind])
        svk = orc.svk(self.m.get("E", 1.0), self.m.get("nu", 0.0))
        self.theta = (np.array([self.m["mu10"], self.m["mu01"], self.m["kappa"]]) if kind == "mr" else
                      np.array([svk.lam, svk.mu]))
        self.rho0 = self.m["rho0"]
        n = 3 * self.N
        if cons == "csr":
            self.rows = csr_rows(self.fixed, self.X, self.N)
            self.targets = self.rows[3] + rng.normal(0.0, 1e-4, len(self.rows[3]))
            nc = len(self.targets)
        else:
            self.targets = self.X[self.fixed] + rng.normal(0.0, 1e-4, (len(self.fixed), 3))
            nc = 3 * len(self.fixed)
        # 5e-4: at 1e-3 one draw in three leaves the Mooney-Rivlin tangent of the beams indefinite (the oracle's Cholesky fails)
        self.x_prev = self.X + rng.normal(0.0, 5e-4, self.X.shape)
        self.v_prev = rng.normal(0.0, 0.2, n)
        self.lam = rng.normal(0.0, 1e3, nc)
        # forces on the gradient coefficients are a hundredth of those on the positions: their rows of M and K are that
        # much lighter (thickness^2 / 12), and a step that inverts an element is not what is differentiated here
        self.f_ext = (rng.normal(0.0, 1e4, (self.N, 3)) * np.where(np.arange(self.N) % 4 == 0, 1.0, 1e-2)[:, None]).reshape(-1)
        self.a = np.array([0.3, -9.81, 2.0])
        # lambda_new moves by rho per unit of x: its weights are scaled by 1 / rho (tests/test_adjoint_np.py)
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
        kind, x, y, z, conn, (L, W, H) = self.prob
        o = orc.AncfOracle(kind, x, y, z, conn, L, W, H, self.material(theta, rho0), fixed=self.fixed)
        o.calc_dsdu_pre()   # both read the reference coefficients, which the targets below then overwrite
        o.calc_mass()
        o.f_ext = f_ext + tnp.mass_times(o.m_off, o.m_col, o.m_val, aad.a_hat(a, self.N))
        anp.set_state(o, x_prev.copy())
        prm = orc.NewtonParams(ATOL, 0.0, 1e-6, RHO, 1, 30, H_STEP)
        if self.cons == "csr":
            o.set_linear_constraints(self.rows[0], self.rows[1], self.rows[2], targets)
            o.v, o.v_prev, o.lam = v_prev.copy(), v_prev.copy(), lam.copy()
            st = o.newton_step_lin(prm)
        else:
            o.xt[self.fixed], o.yt[self.fixed], o.zt[self.fixed] = targets[:, 0], targets[:, 1], targets[:, 2]
            o.v, o.v_prev, o.lam = v_prev.copy(), v_prev.copy(), lam.copy()
            st = o.newton_step(prm)
        assert st[2] < ATOL, f"the oracle's step did not converge: ||g|| = {st[2]:.3e}"
        return o, np.stack([o.x, o.y, o.z], axis=1).reshape(-1), o.v.copy(), o.lam.copy()

    def loss(self, **kw):
        _, x, v, lam = self.step(**kw)
        return self.xbar @ x + self.vbar @ v + self.lambar @ lam

    def central(self, name, direction, eps):
        base = getattr(self, name)
        d = np.asarray(direction, dtype=np.float64).reshape(np.shape(base))
        return (self.loss(**{name: base + eps * d}) - self.loss(**{name: base - eps * d})) / (2.0 * eps)

    def J(self):
        if self.cons == "csr":
            return tnp.csr_J(self.rows[0], self.rows[1], self.rows[2], self.N)
        return tnp.selector_J(self.fixed, self.N)


# Steps of the central differences, from a halving study on beam5 (gap against the restatement at 4, 1, 1/4 times the step;
# truncation falls by 16 per such factor, rounding grows by 4): the vectors move by STEP along a direction whose largest
# component is 1, the moduli by 1e-4 of their size, the acceleration by 0.1 m/s^2, the density by 2.5e-4 of its size.
#   f_ext    8: 2.4e-6   2: 1.5e-7   0.5: 9.6e-9     (truncation: the 100 N of tests/test_adjoint_np.py give 3.9e-5 here)
#   lam      the step is linear in lambda; its derivative is a difference of terms of 1e-10, so only a large step lifts
#            the difference of the loss over its rounding: 1e3: 9e-9, 10: 1.6e-6, 0.6: 3.7e-6
#   x_prev   1e-5: 8.9e-10   2.5e-6: 2.0e-11   6e-7: 7.3e-11
#   v_prev   2e-3: 1.5e-10   5e-4: 1.5e-10
#   targets  1.6e-5: 1.3e-11   4e-6: 2.4e-11   1e-6: 2.4e-10
STEP = dict(f_ext=2.0, v_prev=1e-3, x_prev=2.5e-6, lam=1e3, targets=4e-6)


def differences(p, dirs, shrink=1.0):
    fd = {k: p.central(k, d, shrink * STEP[k] / np.abs(d).max()) for k, d in dirs.items()}
    fd["gravity"] = np.array([p.central("a", np.eye(3)[c], shrink * 0.1) for c in range(3)])
    fd["theta"] = np.array([p.central("theta", np.eye(len(p.theta))[k], shrink * 1e-4 * p.theta[k])
                            for k in range(len(p.theta))])
    fd["rho0"] = p.central("rho0", 1.0, shrink * 2.5e-4 * p.rho0)
    return fd


@functools.lru_cache(maxsize=None)
def build_case(shape, cons, kind):
    """the converged step, its restated adjoint and the central differences of every input, computed once per case"""
    p = Problem(shape, cons, kind)
    o, x, v, lam_new = p.step()
    n = 3 * p.N
    H = aad.dense_H(*(o.assemble_hessian_lin(H_STEP, RHO) if p.cons == "csr" else o.assemble_hessian(H_STEP, RHO)), n)
    J = p.J()
    X1 = x.reshape(-1, 3)
    rng = np.random.default_rng(11)
    dirs = dict(f_ext=rng.normal(size=n), v_prev=rng.normal(size=n), x_prev=rng.normal(size=(p.N, 3)),
                lam=rng.normal(size=len(p.lam)), targets=rng.normal(size=p.targets.shape))
    fd = differences(p, dirs)

    def restated(without_a=False, **kw):
        u = aad.u_vector(v, p.v_prev, H_STEP, p.a, without_a)
        w, out = aad.adjoint_step(H, o, J, H_STEP, RHO, p.xbar, p.vbar, p.lambar, u, p.rho0, **kw)
        pe = aad.sens_per_element(o, X1, w, p.kind)
        got = {k: float(np.dot(out[k].reshape(-1), np.asarray(d).reshape(-1))) for k, d in dirs.items() if k != "lam"}
        got["lam"] = float(out["lam_in"] @ dirs["lam"])
        got["gravity"], got["theta"], got["rho0"] = out["gravity"], pe.sum(axis=0), out["rho0"]
        return w, pe, got
    w, pe, got = restated()
    return dict(p=p, o=o, w=w, pe=pe, got=got, fd=fd, dirs=dirs, restated=restated, x=x)


@pytest.fixture(scope="module", params=[(s, c, k) for s, c in CASES for k in ("svk", "mr")], ids=lambda t: "-".join(t))
def case(request):
    return build_case(*request.param)


def gaps(got, fd):
    """per output: the largest gap over the output's components, relative to its largest component"""
    out = {}
    for k, ref in fd.items():
        g, r = np.atleast_1d(got[k]).astype(float), np.atleast_1d(ref).astype(float)
        out[k] = np.abs(g - r).max() / np.abs(r).max()
    return out


def test_every_output_matches_central_differences(case):
    g = gaps(case["got"], case["fd"])
    p = case["p"]
    for k, v in g.items():
        print(f"{p.shape} {p.cons} {p.kind} {k}: relative gap {v:.3e}")
    bad = {k: v for k, v in g.items() if not v <= BOUND}
    assert not bad, f"adjoint restatement differs from central differences beyond {BOUND}: {bad}"


@pytest.mark.parametrize("kind", ["svk", "mr"])
def test_difference_steps_sit_on_the_plateau(kind):
    """the halving study on the thin shell: with every step halved the gaps stay under the bound too -- were truncation
    what is left of a gap it would have fallen by 4, were it rounding it would have doubled, and neither reaches the bound"""
    c = build_case("plate2x2", "fixed", kind)
    p = c["p"]
    half = gaps(c["got"], differences(p, c["dirs"], shrink=0.5))
    full = gaps(c["got"], c["fd"])
    for k in full:
        print(f"{p.shape} {p.kind} {k}: gap {full[k]:.3e} at the step, {half[k]:.3e} at half of it")
    assert max(half.values()) <= BOUND and max(full.values()) <= BOUND


def test_stiffness_identity_through_the_oracle(case):
    """sum_p theta_p theta_bar_p = -w . f_int against the oracle's own internal force (P is linear in its parameters)"""
    p, o, w = case["p"], case["o"], case["w"]
    lhs = float(p.theta @ case["got"]["theta"])
    f_int = o.internal_force()
    terms = float(np.abs(case["pe"] * p.theta[None, :]).sum() + np.abs(w * f_int).sum())
    print(f"{p.shape} {p.kind}: identity gap {abs(lhs + w @ f_int):.3e} of {terms:.3e}")
    assert abs(lhs + w @ f_int) <= 1e-12 * terms


MISTAKES = {"flipped_w": dict(sign=-1.0), "dropped_jt": dict(drop_jt=True), "a_bar_over_all": dict(all_coefficients=True),
            "u_without_a": dict(without_a=True), "density_without_division": dict(without_division=True)}


@pytest.mark.parametrize("name", sorted(MISTAKES))
def test_the_check_catches_a_wrong_restatement(case, name):
    _, _, wrong = case["restated"](**MISTAKES[name])
    g = gaps(wrong, case["fd"])
    print(case["p"].shape, case["p"].kind, name, {k: f"{v:.2e}" for k, v in g.items()})
    assert max(g.values()) > 100 * BOUND, g
    if name == "dropped_jt":  # every output that reads w is off, not only one
        assert sum(v > BOUND for v in g.values()) >= len(g) // 2, g
