"""Rigid obstacles on ANCF beam and shell meshes on the GPU (DESIGN 3e'): kernel parity with tests/ancf_obstacles_np.py
(pinned without a GPU by tests/test_ancf_obstacles_np.py), exact integration and mesh independence, resting weight,
friction on an incline, the direct and first-order solvers, bitwise checks, the refusals and the tire driver.  Shapes:
one element, a line with shared nodes and an odd count, a 2 x 2 plate (a node of four elements), a 3 x 1 strip."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import ancf_obstacles_np as aonp
from tests import ancf_stress_np as anp
from tests.helpers import csr_to_dense, load_mesh, make_gpu, tl
from tests.test_gpu_ancf_stress import SHAPES, make_ancf_gpu

pytestmark = pytest.mark.gpu
mu = tl.mesh_utils
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
G = 9.81
SOFT = dict(kind="svk", E=1e7, nu=0.3, rho0=1000.0, eta=0.0, lamd=0.0)
PARITY_SHAPES = ("beam1", "beam5", "shell1", "plate2x2", "strip3x1")


def plane(point, normal, kappa, **kw):
    n = np.asarray(normal, dtype=float)
    return tl.RigidPlane(point, n / np.linalg.norm(n), kappa, **kw)


def as_dict(o):
    if isinstance(o, tl.RigidPlane):
        return dict(kind=0, p=o.point, n=o.normal, kappa=o.stiffness, mu=o.friction, eps_v=o.eps_v, vel=o.velocity)
    return dict(kind=1, p=o.center, radius=o.radius, kappa=o.stiffness, mu=o.friction, eps_v=o.eps_v, vel=o.velocity)


def newton(d, h, atol=1e-7, max_inner=40, method=0):
    s = tl.SyncedNewtonSolver(d, 0)
    s.SetParameters(tl.SyncedNewtonParams(atol, 0.0, 1e-6, 1e14, 1, max_inner, h))
    s.SetLinSolveOpts(tl.LinSolveOpts(rel_tol=1e-13, max_iter=50000, method=method))
    return s


def move(d, x):
    d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])


def coefs(d):
    return np.stack(d.RetrievePositionToCPU(), axis=1)


def gravity_load(d, gvec):
    """consistent load of a uniform acceleration: M a with a = gvec on the position coefficients, 0 on the gradients;
    returns (f_ext, total mass)"""
    off, col, val = d.RetrieveMassCSRToCPU()
    a = np.zeros((d.n_coef, 3))
    a[0::4] = np.asarray(gvec)
    f = np.zeros((d.n_coef, 3))
    pos = np.zeros(d.n_coef)
    pos[0::4] = 1.0
    for i in range(d.n_coef):
        f[i] = val[off[i]:off[i + 1]] @ a[col[off[i]:off[i + 1]]]
    mass = float(sum(val[off[i]:off[i + 1]] @ pos[col[off[i]:off[i + 1]]] for i in range(0, d.n_coef, 4)))
    return f.reshape(-1), mass


def scene(shape):
    """A half-space that cuts the left part of the mesh and a sphere that dips into another part from above; friction on
    the half-space for the beams, on the sphere for the shells."""
    prob = SHAPES[shape]()
    beam = prob[0] == 3243
    X = aonp.reference(prob)
    Lx = X[0::4, 0].max()
    if beam:
        obs = [plane([0.5 * Lx, 1.0, 0.0], [0.2, 0.0, 1.0], 3e7, friction=0.4, eps_v=0.5, velocity=[0.2, 0.1, 0.0]),
               tl.RigidSphere([0.7 * Lx, 1.0, 0.05 + 0.2 - 0.03], 0.2, 5e7)]
    else:
        cx = {"shell1": 1.5, "plate2x2": 3.2, "strip3x1": 3.4}[shape]
        obs = [plane([0.375 * Lx, 0.0, 0.0], [0.1, 0.0, 1.0], 3e7),
               tl.RigidSphere([cx, 0.4, 0.05 + 2.0 - 0.08], 2.0, 5e7, friction=0.3, eps_v=0.5, velocity=[0.0, -0.1, 0.05])]
    rng = np.random.default_rng(11)
    xp = X + rng.normal(0, 2e-3, X.shape)
    x = xp + rng.normal(0, 1e-4, X.shape)
    x[0::4] += np.array([0.004, -0.003, 0.0])      # |u| around eps_v h = 5e-3: points on both friction branches
    return prob, obs, xp, x


@functools.lru_cache(maxsize=None)
def parity_reference(shape, h=1e-2):
    """the restated contact terms of a scene: computed once, shared, never modified"""
    prob, obs, xp, x = scene(shape)
    return aonp.assemble(prob, [as_dict(o) for o in obs], x, xp, h)


# ---- 1. parity with the restatement (the tolerances of tests/test_gpu_obstacles.py::test_kernel_parity) ----------------
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_kernel_parity(shape):
    h = 1e-2
    prob, obs, xp, x = scene(shape)
    ref = parity_reference(shape)
    E = prob[4].shape[0]
    assert np.count_nonzero(ref["gap"] < 0) >= E * 32 // 4
    if E > 1:                                       # a one-element mesh cannot have both
        assert not ref["touched"].all()
    out = {}
    for with_obs in (False, True):
        d = make_ancf_gpu(prob, SOFT)
        if with_obs:
            d.SetRigidObstacles(obs)
        s = newton(d, h)
        s.AnalyzeHessianSparsity()
        move(d, xp)
        s.BeginStep()                               # x_prev of the friction term
        move(d, x)
        s.EvalGradient()
        g = s.RetrieveGradientToCPU()
        s.AssembleHessian()
        ro, ci, val = s.RetrieveHessianCSRToCPU()
        out[with_obs] = dict(g=g, H=csr_to_dense(ro, ci, val, 3 * x.shape[0]))
        if with_obs:
            out[True].update(f=d.GetObstacleForces(), w=d.GetSurfacePointWeights(), pts=d.RetrieveContactPointsToCPU(),
                             res=[d.GetObstacleResultant(k) for k in range(2)])
        del s
        d.Destroy()
    got = out[True]
    assert np.allclose(got["w"], ref["weights"], rtol=1e-13, atol=0)
    F = ref["force"].reshape(-1)
    fscale = np.abs(F).max()
    err = {"force": np.max(np.abs(got["f"] - F)) / fscale,
           "g": np.max(np.abs((got["g"] - out[False]["g"]) + F)) / max(fscale, np.abs(out[False]["g"]).max()),
           "H": np.max(np.abs((got["H"] - out[False]["H"]) - ref["hessian"])) / max(np.abs(ref["hessian"]).max(),
                                                                                   np.abs(out[False]["H"]).max()),
           "points": np.max(np.abs(got["pts"][:, :, :3] - ref["points"])) / np.abs(ref["points"]).max(),
           "gap": np.max(np.abs(got["pts"][:, :, 3] - ref["gap"])) / np.abs(ref["gap"]).max(),
           "pressure": np.max(np.abs(got["pts"][:, :, 4] - ref["pressure"])) / ref["pressure"].max()}
    print(shape, {k: f"{v:.2e}" for k, v in err.items()})
    for name, v in err.items():
        assert v <= 1e-13, name
    for k in range(2):
        r, n_act = got["res"][k]
        Fk, cnt = ref["resultants"][k]
        assert np.allclose(r, Fk, rtol=1e-12, atol=1e-12 * fscale)
        assert n_act == cnt


# ---- 2. exact integration and mesh independence ---------------------------------------------------------------------------
def plate_prob(nx, ny, L, W, H=0.1):
    return (3443,) + mu.structured_3443_plate(nx, ny, L, W) + ((L, W, H),)


def beam_prob(n, L):
    gen = mu.GridMeshGenerator(n * L, 0.0, L, True, False)
    gen.generate_mesh()
    return (3243,) + gen.get_coordinates() + (gen.get_element_connectivity(), (L, 0.1, 0.1))


def contact_of(prob, obstacle, x=None):
    """(resultant, points in contact, contact forces [n_coef, 3], coefficients) of one gradient evaluation"""
    d = make_ancf_gpu(prob, SOFT)
    d.SetRigidObstacles([obstacle])
    s = newton(d, 1e-2)
    s.AnalyzeHessianSparsity()
    if x is not None:
        move(d, x)
    s.BeginStep()
    s.EvalGradient()
    r, n = d.GetObstacleResultant(0)
    out = r, n, d.GetObstacleForces().reshape(-1, 3), coefs(d)
    del s
    d.Destroy()
    return out


def test_plate_integrates_exactly():
    """A flat plate pushed a uniform delta into a half-space gives kappa A delta; tilted, with the whole lower face inside
    and the penetration linear in the position, kappa A x the depth at the centroid and the first moment of the depth.
    The 4 x 4 Gauss rule is exact here (degree <= 6 per variable), so the bound is the rounding of 32 .. 128 terms with
    weights that went through the inverse of B: 1e-12, the resultant tolerance of the parity test."""
    kappa, Lx, Ly = 4e7, 4.0, 2.0
    for prob in (plate_prob(1, 1, Lx, Ly), plate_prob(2, 2, Lx / 2, Ly / 2)):
        A = Lx * Ly
        delta = 3e-3
        r, n, _, _ = contact_of(prob, plane([0, 0, -0.05 + delta], [0, 0, 1], kappa))
        assert n == prob[4].shape[0] * 16
        assert abs(r[2] - kappa * A * delta) <= 1e-12 * kappa * A * delta and np.max(np.abs(r[:2])) <= 1e-12 * r[2]
        nrm = np.array([0.004, -0.003, 1.0])
        nrm /= np.linalg.norm(nrm)
        c = np.array([Lx / 2, Ly / 2, -0.05])                       # centre of the lower face
        p0 = c + 0.03 * nrm                                        # depth 0.03 at the centre, > the tilt's 0.01 across the face
        r, n, F, x = contact_of(prob, plane(p0, nrm, kappa))
        assert n == prob[4].shape[0] * 16                           # the upper face stays outside
        assert np.max(np.abs(r - kappa * A * 0.03 * nrm)) <= 1e-12 * kappa * A * 0.03
        # depth(q) = 0.03 - n . (q - c): first moment over the rectangle, then M = kappa int (q - c) depth dA x n
        first = -np.array([nrm[0] * Lx ** 3 * Ly / 12, nrm[1] * Lx * Ly ** 3 / 12, 0.0])
        M_ref = kappa * np.cross(first, nrm)
        M = np.cross(x, F).sum(axis=0) - np.cross(c, r)             # sum_p r_p x f_p = sum_a x_a x F_a
        assert np.max(np.abs(M - M_ref)) <= 1e-12 * kappa * A * 0.03 * Lx


def test_mesh_independence():
    """One shell of twice the size and a 2 x 2 plate on the same rectangle, one beam and a two-element line of the same
    length: the same resultant under a tilted half-space to a few ulps of the sum, 64 EPS x the sum of the absolute terms
    (every term of a component has the sign of the normal's, so that sum is |r|).  The beams' side faces are cut by the
    half-space along a line of constant zeta, which both meshes sample alike."""
    nrm = np.array([0.004, -0.003, 1.0])
    nrm /= np.linalg.norm(nrm)
    pairs = [((plate_prob(1, 1, 4.0, 2.0), plate_prob(2, 2, 2.0, 1.0)), np.array([2.0, 1.0, -0.05])),
             ((beam_prob(1, 1.0), beam_prob(2, 0.5)), np.array([0.5, 1.0, -0.05]))]
    eps = np.finfo(float).eps
    for probs, c in pairs:
        rs = [contact_of(p, plane(c + 0.03 * nrm, nrm, 4e7))[0] for p in probs]
        print(rs, "difference in EPS of the sum:", np.abs(rs[0] - rs[1]) / (eps * np.abs(rs[0])))
        assert np.all(np.abs(rs[0] - rs[1]) <= 64 * eps * np.abs(rs[0]))


# ---- 3. resting weight ---------------------------------------------------------------------------------------------------
def rest(prob, obstacles, gvec=(0.0, 0.0, -G), h=0.05, steps=40, method=0, max_inner=40):
    d = make_ancf_gpu(prob, SOFT)
    f, mass = gravity_load(d, gvec)
    d.SetExternalForce(f)
    d.SetRigidObstacles(obstacles)
    s = newton(d, h, method=method, max_inner=max_inner)
    for _ in range(steps):
        s.Solve()
    return d, s, mass


def test_resting_plate_weight():
    """the tolerance and step count of tests/test_gpu_obstacles.py::test_resting_box_weight"""
    prob = SHAPES["plate2x2"]()
    d, s, mass = rest(prob, [plane([0, 0, -0.05], [0, 0, 1], 1e8)])
    L, W, H = prob[5]
    assert abs(mass - SOFT["rho0"] * 4 * L * W * H) <= 1e-12 * mass
    Wt = mass * G
    r, n_act = d.GetObstacleResultant(0)
    print("plate", r, n_act, Wt)
    assert n_act > 0
    assert abs(r[2] - Wt) <= 1e-8 * Wt
    assert np.max(np.abs(r[:2])) <= 1e-8 * Wt
    del s
    d.Destroy()


def test_beam_across_two_spheres():
    """The two resultants sum to the weight once the beam is at rest.  Backward Euler damps a mode of frequency w by
    1 / sqrt(1 + (w h)^2) per step; the lowest bending mode of the 1.5 m span is w = (pi / 1.5)^2 sqrt(E I / rho A) = 12.7
    rad/s, so h = 0.05 leaves 1e-3 of the initial sag's inertia force after 40 steps and cannot meet 1e-8, while h = 0.2
    (the step of tests/test_gpu_obstacles.py::test_box_on_sphere) leaves 0.37^40 = 1e-17."""
    prob = SHAPES["beam6"]()
    R = 0.5
    obs = [tl.RigidSphere([cx, 1.0, -0.05 - R], R, 1e9, friction=0.5, eps_v=1e-3) for cx in (0.75, 2.25)]
    d, s, mass = rest(prob, obs, h=0.2)
    Wt = mass * G
    (r0, n0), (r1, n1) = d.GetObstacleResultant(0), d.GetObstacleResultant(1)
    print("beam6", r0, n0, r1, n1, Wt)
    assert n0 > 0 and n1 > 0
    assert abs(r0[2] + r1[2] - Wt) <= 1e-8 * Wt
    del s
    d.Destroy()


# ---- 4. friction on an incline (tests/test_gpu_obstacles.py::test_incline with a shell plate) ---------------------------
@pytest.mark.parametrize("fr", [0.6, 0.2])
def test_incline(fr):
    th = math.radians(20.0)
    h, eps_v = 0.02, 1e-3
    d = make_ancf_gpu(SHAPES["plate2x2"](), SOFT)
    f, _ = gravity_load(d, (G * math.sin(th), 0.0, -G * math.cos(th)))
    d.SetExternalForce(f)
    d.SetRigidObstacles([plane([0, 0, -0.05], [0, 0, 1], 1e8, friction=fr, eps_v=eps_v)])
    s = newton(d, h, max_inner=80)
    cx = []
    for _ in range(30):
        s.Solve()
        cx.append(coefs(d)[0::4, 0].mean())
    cx = np.array(cx)
    if fr > math.tan(th):
        creep = np.diff(cx[-6:])
        assert np.all(creep <= eps_v * h)
        assert np.all(creep >= -eps_v * h)
    else:
        a = (cx[-1] - 2 * cx[-2] + cx[-3]) / h ** 2
        expect = G * (math.sin(th) - fr * math.cos(th))
        print("incline", a, expect)
        assert abs(a - expect) <= 0.02 * expect
    del s
    d.Destroy()


# ---- 5. solvers ----------------------------------------------------------------------------------------------------------
def test_direct_equals_iterative():
    obs = [plane([0, 0, -0.05], [0, 0, 1], 1e8, friction=0.3, eps_v=1e-2)]
    xs = []
    for method in (0, 1):
        d, s, _ = rest(SHAPES["plate2x2"](), obs, gvec=(2.0, 0.0, -G), steps=10, method=method)
        xs.append(coefs(d))
        del s
        d.Destroy()
    assert np.max(np.abs(xs[0] - xs[1])) <= 1e-10 * np.max(np.abs(xs[0]))


@pytest.mark.parametrize("solver", ["adamw", "nesterov"])
def test_first_order_solvers_hold_the_weight(solver):
    prob = SHAPES["plate2x2"]()
    obs = [plane([0, 0, -0.05], [0, 0, 1], 1e8)]
    d0, s0, mass = rest(prob, obs)
    xr = coefs(d0)
    del s0
    d0.Destroy()
    Wt = mass * G
    d = make_ancf_gpu(prob, SOFT)
    d.SetExternalForce(gravity_load(d, (0.0, 0.0, -G))[0])
    d.SetRigidObstacles(obs)
    move(d, xr)
    if solver == "adamw":
        s = tl.SyncedAdamWNocoopSolver(d, 0)
        s.SetParameters(tl.SyncedAdamWNocoopParams(max_outer=1, max_inner=50, time_step=1e-3))
    else:
        s = tl.SyncedNesterovSolver(d, 0)
        s.SetParameters(tl.SyncedNesterovParams(max_outer=1, max_inner=20, time_step=1e-3))
    s.Setup()
    s.Solve()
    r, _ = d.GetObstacleResultant(0)
    print(solver, r, Wt)
    assert abs(r[2] - Wt) <= 1e-4 * Wt
    assert np.max(np.abs(coefs(d) - xr)) <= 1e-6
    del s
    d.Destroy()


# ---- 6. bitwise checks ---------------------------------------------------------------------------------------------------
def test_determinism():
    prob, obs, xp, x = scene("plate2x2")
    runs = []
    for _ in range(2):
        d = make_ancf_gpu(prob, SOFT)
        d.SetExternalForce(gravity_load(d, (1.0, 0.0, -G))[0])
        d.SetRigidObstacles(obs)
        move(d, xp)
        s = newton(d, 0.02)
        for _ in range(4):
            s.Solve()
        s.AssembleHessian()
        runs.append((coefs(d), d.GetObstacleForces(), d.GetObstacleResultant(0)[0], d.GetObstacleResultant(1)[0],
                     s.RetrieveHessianCSRToCPU()[2]))
        del s
        d.Destroy()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


def test_set_then_clear_is_bitwise_untouched():
    prob = SHAPES["strip3x1"]()
    xs = []
    for touch in (False, True):
        d = make_ancf_gpu(prob, SOFT)
        d.SetExternalForce(gravity_load(d, (0.0, 0.0, -G))[0])
        if touch:
            d.SetRigidObstacles([plane([0, 0, 0.0], [0, 0, 1], 1e8)])
            d.ClearRigidObstacles()
        s = newton(d, 1e-2)
        s.Solve()
        xs.append((coefs(d), s.RetrieveGradientToCPU()))
        del s
        d.Destroy()
    assert np.array_equal(xs[0][0], xs[1][0])
    assert np.array_equal(xs[0][1], xs[1][1])


@pytest.mark.parametrize("shape", ["beam5", "strip3x1"])
def test_untouched_rows_are_bitwise_the_rows_without_obstacles(shape):
    """Hessian rows of coefficients all of whose elements are untouched: the same bits as without obstacles"""
    prob, obs, xp, x = scene(shape)
    ref = parity_reference(shape)
    ids = aonp.coef_ids(prob)
    free = np.setdiff1d(np.arange(x.shape[0]), ids[ref["touched"]].reshape(-1))
    assert free.size > 0 and free.size < x.shape[0]
    vals = []
    for with_obs in (False, True):
        d = make_ancf_gpu(prob, SOFT)
        if with_obs:
            d.SetRigidObstacles(obs)
        s = newton(d, 1e-2)
        s.AnalyzeHessianSparsity()
        move(d, xp)
        s.BeginStep()
        move(d, x)
        s.EvalGradient()
        s.AssembleHessian()
        vals.append(s.RetrieveHessianCSRToCPU())
        del s
        d.Destroy()
    (ro, ci, v0), (_, _, v1) = vals
    changed = 0
    for i in range(x.shape[0]):
        same = np.array_equal(v0[ro[3 * i]:ro[3 * i + 3]], v1[ro[3 * i]:ro[3 * i + 3]])
        if i in free:
            assert same, i
        changed += not same
    assert changed > 0


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_object_usable():
    lib = tl.load_library()
    prob = SHAPES["plate2x2"]()
    good = plane([0, 0, -0.05], [0, 0, 1], 1e8)
    one = good.to_c()
    # a T10 handle on the ANCF entry points, and the other way round
    X, conn = load_mesh("beam_3x2x1")
    t = make_gpu(X, conn, SOFT)
    assert lib.tlfea_ancf_set_obstacles(t._h, C.byref(one), 1) != 0
    assert "ANCF handles only" in lib.tlfea_last_error().decode()
    t.SetRigidObstacles([plane([0, 0, 0], [0, 0, 1], 1e8)])          # the T10 object still takes its own
    st = newton(t, 1e-2)
    st.Solve()
    assert np.all(np.isfinite(np.stack(t.RetrievePositionToCPU())))
    del st
    t.Destroy()
    # before Setup; the same object is then set up and steps
    kind, x, y, z, conn_a, (L, W, H) = prob
    q = tl.quadrature
    raw = tl.GPU_ANCF3443_Data(len(x) // 4, conn_a.shape[0])
    raw.Initialize()
    with pytest.raises(tl.TlfeaError, match="set up"):
        raw.SetRigidObstacles([good])
    raw.Setup(L, W, H, q.gauss_xi_m_7, q.gauss_eta_m_7, q.gauss_zeta_m_3, q.gauss_xi_4, q.gauss_eta_4, q.gauss_zeta_3,
              q.weight_xi_m_7, q.weight_eta_m_7, q.weight_zeta_m_3, q.weight_xi_4, q.weight_eta_4, q.weight_zeta_3, x, y, z,
              conn_a)
    raw.SetDensity(SOFT["rho0"])
    raw.SetSVK(SOFT["E"], SOFT["nu"])
    with pytest.raises(tl.TlfeaError, match="CalcDsDuPre"):          # set up, but no reference geometry yet
        raw.SetRigidObstacles([good])
    raw.CalcDsDuPre()
    raw.CalcMassMatrix()
    raw.SetRigidObstacles([good])
    sr = newton(raw, 1e-2)
    sr.Solve()
    assert np.all(np.isfinite(coefs(raw)))
    del sr
    raw.Destroy()
    d = make_ancf_gpu(prob, SOFT)
    f, mass = gravity_load(d, (0.0, 0.0, -G))
    d.SetExternalForce(f)
    assert lib.tlfea_t10_set_obstacles(d._h, C.byref(one), 1) != 0
    assert "T10 handles only" in lib.tlfea_last_error().decode()
    arr = (tl.binding.ObstacleC * 17)(*[good.to_c()] * 17)
    assert lib.tlfea_ancf_set_obstacles(d._h, arr, 17) != 0
    assert "0..16" in lib.tlfea_last_error().decode()
    o = good.to_c()
    o.n[2] = 1.0 + 1e-9
    assert lib.tlfea_ancf_set_obstacles(d._h, C.byref(o), 1) != 0
    assert "unit length" in lib.tlfea_last_error().decode()
    d.SetRigidObstacles([good])
    with pytest.raises(tl.TlfeaError, match="outside the 1 obstacles"):
        d.UpdateRigidObstacle(1, good)
    with pytest.raises(tl.TlfeaError, match="outside the 1 obstacles"):
        d.GetObstacleResultant(3)
    v = tl.SyncedVBDSolver(d, 0)
    v.SetParameters(tl.SyncedVBDParams(time_step=1e-2))
    with pytest.raises(tl.TlfeaError, match="rigid obstacles are set"):
        v.Solve()
    del v
    s = newton(d, 0.05)
    nl = np.zeros(d.n_coef, dtype=np.int32)
    lists = tl.binding.HaloListsC()
    ar = tl.binding.ALLREDUCE_FN(lambda u, p, n: 0)
    ex = tl.binding.HALO_EXCHANGE_FN(lambda u, sp, rp, n, pp, so, ro: 0)
    assert lib.tlfea_newton_set_halo(s._h, nl.ctypes.data_as(tl.binding.c_ip), 1, C.byref(lists), ar, ex, None, 1) != 0
    assert "rigid obstacles" in lib.tlfea_last_error().decode()
    with pytest.raises(tl.TlfeaError, match="rigid obstacles"):
        s.SetInterface(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.ones(d.n_coef), lambda p, n: None)
    for _ in range(40):                                              # still usable: the resting scene reaches the weight
        s.Solve()
    r, _ = d.GetObstacleResultant(0)
    assert abs(r[2] - mass * G) <= 1e-8 * mass * G
    del s
    d.Destroy()


# ---- 8. driver -----------------------------------------------------------------------------------------------------------
def test_tire_on_floor_driver(tmp_path):
    exe = os.path.join(HOST, "test_tire_on_floor")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    foot = tmp_path / "footprint.csv"
    p = subprocess.run(["timeout", "-k", "10", "300", exe, "--mesh_dir=" + os.path.join(ROOT, "tests", "golden", "meshes"),
                        "--footprint_path=" + str(foot), "--travel=1.2e-3", "6"], capture_output=True, text=True, timeout=320)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("step ")]
    assert len(rows) == 6
    fz = np.array([float(r[3]) for r in rows])                      # step k floor_force F points n
    assert np.all(fz > 0) and np.all(np.diff(fz) > 0)
    kappa = float([ln for ln in p.stdout.splitlines() if ln.startswith("kappa")][0].split()[1])
    floor = float([ln for ln in p.stdout.splitlines() if ln.startswith("floor")][-1].split()[1])
    pts = np.loadtxt(foot, delimiter=",", skiprows=1)               # x, y, z, gap, pressure
    assert pts.shape[1] == 5 and pts.shape[0] > 0 and np.all(np.isfinite(pts))
    hit = pts[pts[:, 4] > 0]
    assert hit.shape[0] > 0
    assert np.all(np.abs((floor - hit[:, 2]) - hit[:, 4] / kappa) <= 1e-12 * max(1.0, abs(floor)))
