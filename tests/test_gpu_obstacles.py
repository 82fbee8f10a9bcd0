"""Rigid obstacles on the GPU: kernel parity with tests/obstacles_np.py, resting equilibrium against the
weight, rotation invariance, friction on an incline (stick and slide), uniaxial compression between two plates, a
sphere obstacle, the direct and first-order solvers, determinism, the untouched path without obstacles, the refusals
and the rigid-floor driver."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

from tests import obstacles_np as onp
from tests.helpers import csr_to_dense, load_mesh, make_gpu

tl = importlib.import_module("total-lagrangian-fea_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
G = 9.81
SOFT = dict(kind="svk", E=1e7, nu=0.3, rho0=1000.0, eta=0.0, lamd=0.0)


def body(X, conn, gravity=(0.0, 0.0, -G), m=SOFT):
    """An object with gravity as f_ext = (row sums of M) g; returns (data, nodal masses)."""
    d = make_gpu(X, conn, m)
    off, _, val = d.RetrieveMassCSRToCPU()
    mass = np.add.reduceat(val, off[:-1])
    d.SetExternalForce((mass[:, None] * np.asarray(gravity)[None, :]).reshape(-1))
    return d, mass


def newton(d, h, atol=1e-7, max_inner=40, method=0):
    s = tl.SyncedNewtonSolver(d, 0)
    s.SetParameters(tl.SyncedNewtonParams(atol, 0.0, 1e-6, 1e14, 1, max_inner, h))
    s.SetLinSolveOpts(tl.LinSolveOpts(rel_tol=1e-13, max_iter=50000, method=method))
    return s


def positions(d):
    return np.stack(d.RetrievePositionToCPU(), axis=1)


def plane(point, normal, kappa, **kw):
    n = np.asarray(normal, dtype=float)
    return tl.RigidPlane(point, n / np.linalg.norm(n), kappa, **kw)


def as_dict(o):
    if isinstance(o, tl.RigidPlane):
        return dict(kind=0, p=o.point, n=o.normal, kappa=o.stiffness, mu=o.friction, eps_v=o.eps_v, vel=o.velocity)
    return dict(kind=1, p=o.center, radius=o.radius, kappa=o.stiffness, mu=o.friction, eps_v=o.eps_v, vel=o.velocity)


def rest(X, conn, obstacles, h=0.05, steps=40, gravity=(0.0, 0.0, -G), method=0, m=SOFT):
    d, mass = body(X, conn, gravity, m)
    d.SetRigidObstacles(obstacles)
    s = newton(d, h, method=method)
    for _ in range(steps):
        s.Solve()
    return d, s, mass


# ---- 1. kernel parity ----------------------------------------------------------------------------------------------
def test_kernel_parity():
    X, conn = load_mesh("res2")
    rng = np.random.default_rng(3)
    h = 1e-2
    obs = [plane([0, 0, 0.05], [0.01, 0.005, 1.0], 3e7, friction=0.4, eps_v=0.5, velocity=[0.2, 0.1, 0.0]),
           tl.RigidSphere([3.1, 2.1, 1.1], 0.35, 5e7, friction=0.3, eps_v=0.5, velocity=[0.0, -0.1, 0.05])]
    xp = X + rng.normal(0, 2e-2, X.shape)
    x = xp + rng.normal(0, 5e-3, X.shape)
    out = {}
    for with_obs in (False, True):
        d, _ = body(X, conn)
        if with_obs:
            d.SetRigidObstacles(obs)
        s = newton(d, h)
        s.AnalyzeHessianSparsity()
        d.UpdatePositions(xp[:, 0], xp[:, 1], xp[:, 2])
        s.BeginStep()                                   # x_prev of the friction term
        d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])
        s.EvalGradient()
        g = s.RetrieveGradientToCPU()
        s.AssembleHessian()
        ro, ci, val = s.RetrieveHessianCSRToCPU()
        out[with_obs] = (g, csr_to_dense(ro, ci, val, 3 * X.shape[0]), d.GetObstacleForces() if with_obs else None,
                         d.GetSurfaceWeights(), [d.GetObstacleResultant(k) for k in range(2)] if with_obs else None)
        del s
        d.Destroy()
    w = out[True][3]
    assert np.allclose(w, onp.surface_weights(X, conn), rtol=1e-13, atol=0)
    F, B = onp.nodal([as_dict(o) for o in obs], w, x, xp, h)
    assert np.count_nonzero(np.linalg.norm(F, axis=1)) > 20
    fscale = np.abs(F).max()
    assert np.max(np.abs(out[True][2] - F.reshape(-1))) <= 1e-13 * fscale
    assert np.max(np.abs((out[True][0] - out[False][0]) + F.reshape(-1))) <= 1e-13 * max(fscale, np.abs(out[False][0]).max())
    dH = out[True][1] - out[False][1]
    N = X.shape[0]
    bscale = h * np.abs(B).max()
    for i in range(N):
        assert np.max(np.abs(dH[3 * i:3 * i + 3, 3 * i:3 * i + 3] - h * B[i])) <= 1e-13 * bscale
        dH[3 * i:3 * i + 3, 3 * i:3 * i + 3] = 0.0
    assert np.max(np.abs(dH)) <= 1e-13 * np.abs(out[False][1]).max()   # nothing off the diagonal blocks
    # resultants: per obstacle, fixed-order sum of its shares
    for k, o in enumerate(obs):
        Fk, _ = onp.nodal([as_dict(o)], w, x, xp, h)
        r, n_act = out[True][4][k]
        assert np.allclose(r, Fk.sum(axis=0), rtol=1e-12, atol=1e-12 * fscale)
        dist = np.array([onp.distance(as_dict(o), x[i])[0] for i in range(N)])
        assert n_act == int(np.count_nonzero((dist < 0) & (w > 0)))


# ---- 2. resting equilibrium -----------------------------------------------------------------------------------------
def test_resting_box_weight():
    X, conn = load_mesh("beam_3x2x1")
    kappa = 1e8
    d, s, mass = rest(X, conn, [plane([0, 0, 0], [0, 0, 1], kappa)])
    W = mass.sum() * G
    r, n_act = d.GetObstacleResultant(0)
    assert n_act > 0
    assert abs(r[2] - W) <= 1e-8 * W
    assert np.max(np.abs(r[:2])) <= 1e-8 * W
    x = positions(d)
    w = d.GetSurfaceWeights()
    pen = np.sum(w * np.maximum(-x[:, 2], 0.0))
    assert abs(pen - W / kappa) <= 1e-8 * W / kappa
    d.Destroy()


# ---- 3. rotation invariance -----------------------------------------------------------------------------------------
def test_rotation_invariance():
    X, conn = load_mesh("beam_3x2x1")
    rng = np.random.default_rng(5)
    A = rng.normal(size=(3, 3))
    R, _ = np.linalg.qr(A)
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    obs0 = plane([0, 0, 0], [0, 0, 1], 1e8)
    d0, _, _ = rest(X, conn, [obs0], steps=20)
    x0 = positions(d0)
    d1, _, _ = rest(X @ R.T, conn, [plane([0, 0, 0], R @ np.array([0, 0, 1.0]), 1e8)], steps=20,
                    gravity=tuple(R @ np.array([0, 0, -G])))
    x1 = positions(d1)
    assert np.max(np.abs(x1 - x0 @ R.T)) <= 1e-9 * np.max(np.abs(x0))
    d0.Destroy()
    d1.Destroy()


# ---- 4. friction on an incline --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", [0.6, 0.2])
def test_incline(mu):
    X, conn = load_mesh("beam_3x2x1")
    th = math.radians(20.0)
    h, eps_v = 0.02, 1e-3
    d, _ = body(X, conn, gravity=(G * math.sin(th), 0.0, -G * math.cos(th)))
    d.SetRigidObstacles([plane([0, 0, 0], [0, 0, 1], 1e8, friction=mu, eps_v=eps_v)])
    s = newton(d, h, max_inner=80)
    cx = []
    for _ in range(30):
        s.Solve()
        cx.append(positions(d)[:, 0].mean())
    cx = np.array(cx)
    if mu > math.tan(th):
        creep = np.diff(cx[-6:])
        assert np.all(creep <= eps_v * h)
        assert np.all(creep >= -eps_v * h)
    else:
        a = (cx[-1] - 2 * cx[-2] + cx[-3]) / h ** 2
        expect = G * (math.sin(th) - mu * math.cos(th))
        assert abs(a - expect) <= 0.02 * expect
    d.Destroy()


# ---- 5. uniaxial compression between two frictionless plates --------------------------------------------------------
def test_uniaxial_compression():
    X, conn = tl.mesh_utils.structured_t10_box(2, 2, 3, 1.0, 1.0, 1.5)
    E, Lz = 1e7, 1.5
    m = dict(SOFT, E=E, nu=0.3)
    d, _ = body(X, conn, gravity=(0.0, 0.0, 0.0), m=m)
    kappa = 1e11
    top = lambda z: plane([0, 0, z], [0, 0, -1], kappa)                # noqa: E731
    d.SetRigidObstacles([plane([0, 0, 0], [0, 0, 1], kappa), top(Lz)])
    s = newton(d, 1.0, atol=1e-6)
    travel = 2e-3 * Lz
    for k in range(1, 11):
        d.UpdateRigidObstacle(1, top(Lz - travel * min(k, 5) / 5))
        s.Solve()
    x = positions(d)
    bot, topn = X[:, 2] < 1e-9, X[:, 2] > Lz - 1e-9
    strain = 1.0 - (x[topn, 2].mean() - x[bot, 2].mean()) / Lz
    r, _ = d.GetObstacleResultant(1)
    expect = E * 1.0 * strain
    assert strain > 1e-3
    assert abs(-r[2] - expect) <= 0.01 * expect
    r0, _ = d.GetObstacleResultant(0)
    assert abs(r0[2] + r[2]) <= 1e-6 * abs(r[2])
    d.Destroy()


# ---- 6. sphere obstacle ---------------------------------------------------------------------------------------------
def test_box_on_sphere():
    X, conn = load_mesh("beam_3x2x1")
    Rs = 20.0
    d, s, mass = rest(X, conn, [tl.RigidSphere([1.5, 1.0, -Rs], Rs, 1e9)], h=0.2)
    W = mass.sum() * G
    r, n_act = d.GetObstacleResultant(0)
    assert n_act > 0
    assert abs(r[2] - W) <= 1e-8 * W
    d.Destroy()


# ---- 7. solvers -----------------------------------------------------------------------------------------------------
def test_direct_equals_iterative():
    X, conn = load_mesh("beam_3x2x1")
    obs = [plane([0, 0, 0], [0, 0, 1], 1e8, friction=0.3, eps_v=1e-2)]
    xs = []
    for method in (0, 1):
        d, s, _ = rest(X, conn, obs, steps=10, gravity=(2.0, 0.0, -G), method=method)
        xs.append(positions(d))
        d.Destroy()
    assert np.max(np.abs(xs[0] - xs[1])) <= 1e-10 * np.max(np.abs(xs[0]))


@pytest.mark.parametrize("solver", ["adamw", "nesterov"])
def test_first_order_solvers_hold_the_weight(solver):
    X, conn = load_mesh("beam_3x2x1")
    obs = [plane([0, 0, 0], [0, 0, 1], 1e8)]
    d0, _, mass = rest(X, conn, obs)
    xr = positions(d0)
    d0.Destroy()
    W = mass.sum() * G
    d, _ = body(X, conn)
    d.SetRigidObstacles(obs)
    d.UpdatePositions(xr[:, 0], xr[:, 1], xr[:, 2])
    if solver == "adamw":
        s = tl.SyncedAdamWNocoopSolver(d, 0)
        s.SetParameters(tl.SyncedAdamWNocoopParams(max_outer=1, max_inner=50, time_step=1e-3))
    else:
        s = tl.SyncedNesterovSolver(d, 0)
        s.SetParameters(tl.SyncedNesterovParams(max_outer=1, max_inner=20, time_step=1e-3))
    s.Setup()
    s.Solve()
    r, _ = d.GetObstacleResultant(0)
    assert abs(r[2] - W) <= 1e-4 * W
    assert np.max(np.abs(positions(d) - xr)) <= 1e-6
    del s
    d.Destroy()


# ---- 8. determinism -------------------------------------------------------------------------------------------------
def test_determinism():
    X, conn = load_mesh("res2")
    obs = [plane([0, 0, 0], [0.05, 0, 1], 1e8, friction=0.4, eps_v=1e-2), tl.RigidSphere([1.5, 1.0, 1.8], 0.5, 1e8)]
    runs = []
    for _ in range(2):
        d, s, _ = rest(X, conn, obs, h=0.02, steps=8, gravity=(1.0, 0.0, -G))
        runs.append((positions(d), d.GetObstacleForces(), d.GetObstacleResultant(0)[0]))
        d.Destroy()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


# ---- 9. nothing changes without obstacles ---------------------------------------------------------------------------
def test_set_then_clear_is_bitwise_untouched():
    X, conn = load_mesh("beam_3x2x1")
    xs = []
    for touch in (False, True):
        d, _ = body(X, conn)
        if touch:
            d.SetRigidObstacles([plane([0, 0, 0.5], [0, 0, 1], 1e8)])
            d.ClearRigidObstacles()
        s = newton(d, 1e-2)
        s.Solve()
        xs.append((positions(d), s.RetrieveGradientToCPU()))
        d.Destroy()
    assert np.array_equal(xs[0][0], xs[1][0])
    assert np.array_equal(xs[0][1], xs[1][1])


# ---- 10. refusals ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_object_usable():
    X, conn = load_mesh("beam_3x2x1")
    d, mass = body(X, conn)
    lib = tl.load_library()
    good = plane([0, 0, 0], [0, 0, 1], 1e8)
    bad = []
    for field, value in (("stiffness", 0.0), ("friction", -1.0), ("eps_v", 0.0), ("kind", 7)):
        o = good.to_c()
        setattr(o, field, value)
        bad.append((o, field if field != "kind" else "unknown kind"))
    o = good.to_c()
    o.n[2] = 1.0 + 1e-9
    bad.append((o, "unit length"))
    o = tl.RigidSphere([0, 0, 0], 1.0, 1e8).to_c()
    o.radius = 0.0
    bad.append((o, "radius"))
    for o, msg in bad:
        assert lib.tlfea_t10_set_obstacles(d._h, C.byref(o), 1) != 0
        assert msg in lib.tlfea_last_error().decode()
    arr = (tl.binding.ObstacleC * 17)(*[good.to_c()] * 17)
    assert lib.tlfea_t10_set_obstacles(d._h, arr, 17) != 0
    assert "0..16" in lib.tlfea_last_error().decode()
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
    nl = np.zeros(X.shape[0], dtype=np.int32)
    lists = tl.binding.HaloListsC()
    ar = tl.binding.ALLREDUCE_FN(lambda u, p, n: 0)
    ex = tl.binding.HALO_EXCHANGE_FN(lambda u, sp, rp, n, pp, so, ro: 0)
    assert lib.tlfea_newton_set_halo(s._h, nl.ctypes.data_as(tl.binding.c_ip), 1, C.byref(lists), ar, ex, None, 1) != 0
    assert "rigid obstacles" in lib.tlfea_last_error().decode()
    with pytest.raises(tl.TlfeaError, match="rigid obstacles"):
        s.SetInterface(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.ones(X.shape[0]), lambda p, n: None)
    # still usable: the resting scene reaches the weight
    for _ in range(40):
        s.Solve()
    r, _ = d.GetObstacleResultant(0)
    assert abs(r[2] - mass.sum() * G) <= 1e-8 * mass.sum() * G
    del s
    d.Destroy()


# ---- 11. driver -----------------------------------------------------------------------------------------------------
def test_rigid_floor_driver(tmp_path):
    exe = os.path.join(HOST, "test_sphere_drop_rigid_floor")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    csv = tmp_path / "floor.csv"
    p = subprocess.run(["timeout", "-k", "10", "600", exe, "--mesh_dir=" + os.path.join(ROOT, "tests", "golden", "meshes"),
                        "--csv_path=" + str(csv), "300", "0"],
                       capture_output=True, text=True, timeout=620)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = np.loadtxt(csv, delimiter=",", skiprows=1)
    assert rows.shape[0] == 300
    assert np.all(np.isfinite(rows))
    weight = float([ln for ln in p.stdout.splitlines() if ln.startswith("weight")][0].split()[1])
    assert abs(rows[-1, 2] - weight) <= 0.01 * weight
