"""Distributed loads on the GPU: gravity on any element kind, dead traction and follower pressure on ANCF beam
and shell meshes, against tests/ancf_loads_np.py (pinned without a GPU by tests/test_ancf_loads_np.py).  Kernel parity,
bitwise checks, constant loads against the same vector through SetExternalForce (the path the oracle pins), the fixed
point of a follower-pressure step, T10 gravity, the refusals and the inflation driver.  Shapes: one element, a line with
shared nodes and an odd count, a 2 x 2 plate (a node of four elements), a 3 x 1 strip."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import ancf_loads_np as lnp
from tests import ancf_obstacles_np as aonp
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_gpu, make_oracle, tl
from tests.test_gpu_ancf_stress import SHAPES

pytestmark = pytest.mark.gpu
Q = tl.quadrature
EPS = np.finfo(float).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
SOFT = dict(kind="svk", E=1e7, nu=0.3, rho0=1000.0, eta=0.0, lamd=0.0)
LOAD_SHAPES = ("beam1", "beam5", "shell1", "plate2x2", "strip3x1")
A_G = np.array([0.3, -0.2, -9.81])
T_VEC = np.array([120.0, -80.0, 300.0])


def build(prob, fixed=None, mass=True, dsdu=True):
    """the call order of tests/test_gpu_ancf.py::make_pair"""
    kind, x, y, z, conn, (L, W, H) = prob
    d = (tl.GPU_ANCF3243_Data if kind == 3243 else tl.GPU_ANCF3443_Data)(len(x) // 4, conn.shape[0])
    d.Initialize()
    if fixed is not None:
        d.SetNodalFixed(fixed)
    if kind == 3243:
        d.Setup(L, W, H, Q.gauss_xi_m_6, Q.gauss_xi_3, Q.gauss_eta_2, Q.gauss_zeta_2, Q.weight_xi_m_6, Q.weight_xi_3,
                Q.weight_eta_2, Q.weight_zeta_2, x, y, z, conn)
    else:
        d.Setup(L, W, H, Q.gauss_xi_m_7, Q.gauss_eta_m_7, Q.gauss_zeta_m_3, Q.gauss_xi_4, Q.gauss_eta_4, Q.gauss_zeta_3,
                Q.weight_xi_m_7, Q.weight_eta_m_7, Q.weight_zeta_m_3, Q.weight_xi_4, Q.weight_eta_4, Q.weight_zeta_3,
                x, y, z, conn)
    d.SetDensity(SOFT["rho0"])
    d.SetDamping(0.0, 0.0)
    d.SetSVK(SOFT["E"], SOFT["nu"])
    if dsdu:
        d.CalcDsDuPre()
    if mass:
        d.CalcMassMatrix()
    if fixed is not None:
        d.CalcConstraintData()
        d.ConvertToCSR_ConstraintJacT()
        d.BuildConstraintJacobianCSR()
    return d


def newton(d, h, atol=1e-7, max_inner=40, method=0, rho=1e14):
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(atol, 0.0, 1e-6, rho, 1, max_inner, h))
    s.SetLinSolveOpts(tl.LinSolveOpts(rel_tol=1e-13, max_iter=50000, method=method))
    return s


def move(d, x):
    d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])


def coefs(d):
    return np.stack(d.RetrievePositionToCPU(), axis=1)


def close_positions(xa, xb, x0):
    """the project's rule for two runs of one step: 1e-10 of the displacement + 8 ulp of the coordinates"""
    disp = np.abs(xa - x0).max()
    err = np.abs(xa - xb).max()
    print(f"  displacement {disp:.3e}  difference {err:.3e}")
    return err <= 1e-10 * disp + 8 * EPS * np.abs(x0).max()


def scene(shape):
    """perturbed coefficients (as scene() of the obstacle tests) and the load sets of the parity test: each kind alone and
    all three together; the pressure loads put two faces on element 0, and on `plate2x2` every element is loaded, so the
    node of four elements is in the set"""
    prob = SHAPES[shape]()
    X = aonp.reference(prob)
    x = X + np.random.default_rng(11).normal(0, 2e-3, X.shape)
    E, nf = prob[4].shape[0], lnp.FACES[prob[0]]
    el = list(range(E))
    trac = [dict(kind=0, face=nf - 1, elems=el, value=T_VEC, scale=1.5),
            dict(kind=0, face=0, elems=el[::2], value=-0.5 * T_VEC, scale=1.0)]
    press = [dict(kind=1, face=nf - 1, elems=el, value=3e4, scale=0.75),
             dict(kind=1, face=0, elems=[0], value=-1.2e4, scale=1.0),
             dict(kind=1, face=nf - 1, elems=el[::2], value=5e3, scale=2.0)]      # a second load on the same faces
    sets = {"gravity": (A_G, []), "traction": (None, trac), "pressure": (None, press), "all": (A_G, trac + press)}
    return prob, x, sets


def apply(d, gravity, loads):
    if gravity is not None:
        d.SetGravity(gravity)
    for ld in loads:
        if ld["kind"] == 0:
            d.AddSurfaceTraction(ld["face"], ld["elems"], ld["value"], ld["scale"])
        else:
            d.AddFollowerPressure(ld["face"], ld["elems"], ld["value"], ld["scale"])


@functools.lru_cache(maxsize=None)
def parity_reference(shape, which):
    """the restated load of a scene: computed once, shared, never modified"""
    prob, x, sets = scene(shape)
    g, loads = sets[which]
    return lnp.total(prob, x, SOFT["rho0"], g, loads)


# ---- 1. parity with the restatement (the bound of the obstacle parity tests) ---------------------------------------------
@pytest.mark.parametrize("shape", LOAD_SHAPES)
def test_kernel_parity(shape):
    """Measured on the MI355X (largest over the four load sets): see DESIGN 3h."""
    prob, x, sets = scene(shape)
    d = build(prob)
    s = newton(d, 1e-2)
    s.AnalyzeHessianSparsity()
    move(d, x)
    s.BeginStep()
    s.EvalGradient()
    g0 = s.RetrieveGradientToCPU()
    assert not d.GetLoadForces().any()
    for which, (g, loads) in sets.items():
        apply(d, g, loads)
        s.EvalGradient()
        f, g1 = d.GetLoadForces(), s.RetrieveGradientToCPU()
        ref = parity_reference(shape, which)
        scale = np.abs(ref).max()
        err = np.abs(f.reshape(-1, 3) - ref).max() / scale
        err_g = np.abs((g1 - g0) + f).max() / max(scale, np.abs(g0).max())
        res = d.GetLoadResultant()
        print(shape, which, f"force {err:.2e}  gradient {err_g:.2e}")
        assert err <= 1e-13
        assert err_g <= 1e-13
        assert np.abs(res - ref[0::4].sum(axis=0)).max() <= 1e-12 * np.abs(ref[0::4]).sum()
        d.ClearLoads()
    del s
    d.Destroy()


# ---- 2. bitwise ----------------------------------------------------------------------------------------------------------------
def test_bitwise():
    prob, x, sets = scene("plate2x2")
    g, loads = sets["all"]

    def run(mode):
        d = build(prob)
        if mode in ("loaded", "cleared", "scale0"):
            apply(d, g if mode != "scale0" else None, loads if mode != "scale0" else [ld for ld in loads if ld["kind"] == 1])
        if mode == "cleared":
            d.ClearLoads()
        if mode == "scale0":
            for k in range(3):
                d.SetLoadScale(k, 0.0)
        s = newton(d, 1e-2)
        move(d, x)
        s.BeginStep()
        s.EvalGradient()
        out = [s.RetrieveGradientToCPU(), d.GetLoadForces()]
        s.EvalGradient()
        out += [s.RetrieveGradientToCPU(), d.GetLoadForces()]
        s.Solve()
        out.append(coefs(d))
        del s
        d.Destroy()
        return out

    a, b, never, cleared, zero = run("loaded"), run("loaded"), run("never"), run("cleared"), run("scale0")
    assert np.array_equal(a[0], a[2]) and np.array_equal(a[1], a[3])         # two evaluations
    assert all(np.array_equal(p, q) for p, q in zip(a, b))                   # two objects
    assert a[1].any() and not np.array_equal(a[4], never[4])
    assert all(np.array_equal(p, q) for p, q in zip(cleared, never))         # set, clear and step = never set
    assert np.array_equal(zero[0], never[0]) and np.array_equal(zero[4], never[4]) and not zero[1].any()


# ---- 3. constant loads in a step: the same vector through SetExternalForce ----------------------------------------------------
def clamp_left(prob):
    """the coefficients of the nodes at x = 0"""
    X = aonp.reference(prob)
    nodes = np.where(np.abs(X[0::4, 0]) < 1e-12)[0]
    return (4 * nodes[:, None] + np.arange(4)[None, :]).reshape(-1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def strip_dead_load():
    prob = SHAPES["strip3x1"]()
    el = list(range(prob[4].shape[0]))
    return lnp.total(prob, None, SOFT["rho0"], A_G, [dict(kind=0, face=1, elems=el, value=T_VEC, scale=1.0)]).reshape(-1)


@pytest.mark.parametrize("method", [0, 1])
def test_constant_loads_step_like_external_force(method):
    prob = SHAPES["strip3x1"]()
    el = list(range(prob[4].shape[0]))
    X = aonp.reference(prob)
    out = {}
    for how in ("loads", "f_ext"):
        d = build(prob, fixed=clamp_left(prob))
        if how == "loads":
            d.SetGravity(A_G)
            d.AddSurfaceTraction(1, el, T_VEC)
        else:
            d.SetExternalForce(strip_dead_load())
        s = newton(d, 1e-2, atol=1e-6, method=method, rho=1e10)     # rho: see test_follower_pressure_step_is_a_fixed_point
        counts = []
        for _ in range(3):
            s.Solve()
            counts.append(s.GetStats()["newton"])
        out[how] = (coefs(d), counts)
        if how == "loads":
            assert np.array_equal(d.RetrieveExternalForceToCPU(), np.zeros(3 * d.n_coef))  # beside f_ext, not in it
        del s
        d.Destroy()
    print(method, out["loads"][1], out["f_ext"][1])
    assert out["loads"][1] == out["f_ext"][1] and max(out["loads"][1]) < 40          # converged, in the same iterations
    assert close_positions(out["loads"][0], out["f_ext"][0], X)


def test_nesterov_takes_the_loads_through_the_same_evaluation():
    prob = SHAPES["beam5"]()
    X = aonp.reference(prob)
    f = lnp.gravity_force(prob, SOFT["rho0"], A_G).reshape(-1)
    out = {}
    for how in ("loads", "f_ext"):
        d = build(prob)
        if how == "loads":
            d.SetGravity(A_G)
        else:
            d.SetExternalForce(f)
        s = tl.SyncedNesterovSolver(d, 0)
        s.SetParameters(tl.SyncedNesterovParams(max_outer=1, max_inner=20, time_step=1e-3))
        s.Setup()
        s.Solve()
        out[how] = coefs(d)
        del s
        d.Destroy()
    assert np.abs(out["loads"] - X).max() > 0
    assert close_positions(out["loads"], out["f_ext"], X)


# ---- 4. follower pressure in a step: fixed-point consistency ---------------------------------------------------------------------
def test_follower_pressure_step_is_a_fixed_point():
    """H lacks the load stiffness, so Newton converges linearly in the pressure term and is given more inner iterations.
    The clamp's penalty term h rho c is rounded at h rho x 2.2e-16 on a clamped coefficient of value 1: 2e-4 with the
    rho = 1e14 of the other tests, a floor under |g| that no inner_atol below it can certify.  rho = 1e8 puts the floor at
    1e-9.  First the count: a step to inner_atol = 1e-8 (1e-11 of the load's rows), convergence asserted.  Then the fixed
    point: the position rule is 1e-10 of a 1e-3 displacement, and a residual of 1e-8 over a stiffness M / h of 1e3 and
    less would use it up, so both runs of the comparison iterate to the floor (inner_atol below it, a fixed count well
    past the measured one) and |g| <= 1e-8 is asserted on both.  Measured counts: DESIGN 3h."""
    prob = SHAPES["strip3x1"]()
    el = list(range(prob[4].shape[0]))
    X = aonp.reference(prob)
    h, atol, p, rho, n_fix = 1e-2, 1e-8, 1e3, 1e8, 30
    for with_p in (False, True):
        d = build(prob, fixed=clamp_left(prob))
        if with_p:
            d.AddFollowerPressure(1, el, p)
        else:
            d.SetExternalForce(lnp.pressure_force(prob, X, 1, el, p).reshape(-1))     # the same load, frozen
        s = newton(d, h, atol=atol, max_inner=100, rho=rho)
        s.Solve()
        st = s.GetStats()
        print("follower pressure:" if with_p else "frozen load:", st)
        assert st["norm_g"] <= atol and st["newton"] < n_fix
        del s
        d.Destroy()
    d = build(prob, fixed=clamp_left(prob))
    d.AddFollowerPressure(1, el, p)
    s = newton(d, h, atol=1e-13, max_inner=n_fix, rho=rho)
    s.Solve()
    st = s.GetStats()
    print("to the floor, follower pressure:", st)
    assert st["norm_g"] <= atol
    xs, fs = coefs(d), d.GetLoadForces()
    ref = lnp.pressure_force(prob, xs, 1, el, p)
    assert np.abs(fs.reshape(-1, 3) - ref).max() <= 1e-13 * np.abs(ref).max()    # the load of the converged coefficients
    del s
    d.Destroy()
    d = build(prob, fixed=clamp_left(prob))
    d.SetExternalForce(fs)
    s = newton(d, h, atol=1e-13, max_inner=n_fix, rho=rho)
    s.Solve()
    st2 = s.GetStats()
    print("to the floor, f* as f_ext:", st2)
    assert st2["norm_g"] <= atol
    assert close_positions(xs, coefs(d), X)
    del s
    d.Destroy()
    tip = np.where(np.abs(X[0::4, 0] - X[0::4, 0].max()) < 1e-12)[0]
    assert np.all(xs[4 * tip, 2] - X[4 * tip, 2] < 0)                             # top face, normal +z: bends toward -z


# ---- 5. T10: the body force alone -------------------------------------------------------------------------------------------------
def test_t10_gravity():
    Xn, conn = load_mesh("beam_3x2x1")
    m = MATERIALS["svk"]
    fixed = fixed_x0(Xn)
    o = make_oracle(Xn, conn, m, fixed)
    M = np.zeros((Xn.shape[0], Xn.shape[0]))
    for i in range(Xn.shape[0]):
        M[i, o.m_col[o.m_off[i]:o.m_off[i + 1]]] = o.m_val[o.m_off[i]:o.m_off[i + 1]]
    ref = M @ np.tile(A_G, (Xn.shape[0], 1))
    out = {}
    for how in ("loads", "f_ext"):
        d = make_gpu(Xn, conn, m, fixed, None if how == "loads" else ref.reshape(-1))
        if how == "loads":
            d.SetGravity(A_G)
        s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
        s.SetParameters(tl.SyncedNewtonParams(1e-6, 0.0, 1e-6, 1e14, 5, 10, 1e-3))
        s.SetLinSolveOpts(tl.LinSolveOpts(1e-13, 20000, 10))
        if how == "loads":
            s.EvalGradient()
            f = d.GetLoadForces().reshape(-1, 3)
            err = np.abs(f - ref).max() / np.abs(ref).max()
            print(f"T10 gravity {err:.2e}")
            assert err <= 1e-13
            assert np.abs(d.GetLoadResultant() - ref.sum(axis=0)).max() <= 1e-12 * np.abs(ref).sum()
        s.Solve()
        out[how] = (coefs(d), s.GetStats()["newton"])
        del s
        d.Destroy()
    assert out["loads"][1] == out["f_ext"][1]
    assert close_positions(out["loads"][0], out["f_ext"][0], Xn)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def c_load(kind, face, elems, value=(1e3, 0.0, 0.0), scale=1.0):
    e = np.ascontiguousarray(elems, dtype=np.int32)
    return tl.binding.SurfaceLoadC(kind, face, tuple(value), scale, tl.binding.ip(e), int(e.size)), e


def test_refusals_leave_the_object_usable():
    lib = tl.load_library()
    err = lambda: lib.tlfea_last_error().decode()
    prob = SHAPES["plate2x2"]()
    one, keep = c_load(1, 1, [0, 1])
    # surface loads on a T10 handle; its body acceleration needs the mass matrix
    Xn, conn = load_mesh("beam_3x2x1")
    t = make_gpu(Xn, conn, MATERIALS["svk"])
    assert lib.tlfea_ancf_set_surface_loads(t._h, C.byref(one), 1) != 0 and "ANCF handles only" in err()
    assert lib.tlfea_ancf_update_load_scale(t._h, 0, 1.0) != 0 and "ANCF handles only" in err()
    t.SetGravity(A_G)
    t.Destroy()
    # before Setup, before CalcDsDuPre, before CalcMassMatrix
    kind, x, y, z, conn_a, _ = prob
    raw = tl.GPU_ANCF3443_Data(len(x) // 4, conn_a.shape[0])
    raw.Initialize()
    with pytest.raises(tl.TlfeaError, match="set up"):
        raw.AddFollowerPressure(1, [0], 1e3)
    with pytest.raises(tl.TlfeaError, match="set up"):
        raw.SetGravity(A_G)
    raw.Destroy()
    raw = build(prob, mass=False, dsdu=False)
    with pytest.raises(tl.TlfeaError, match="CalcDsDuPre"):
        raw.AddSurfaceTraction(1, [0], T_VEC)
    with pytest.raises(tl.TlfeaError, match="CalcDsDuPre"):
        raw.SetGravity(A_G)
    raw.CalcDsDuPre()
    with pytest.raises(tl.TlfeaError, match="CalcMassMatrix"):
        raw.SetGravity(A_G)
    raw.AddSurfaceTraction(1, [0], T_VEC)                                # surface loads need no mass matrix
    raw.Destroy()
    # the list checks of the C-ABI (the mirror refuses the same earlier: tests/test_ancf_loads_np.py)
    d = build(prob)
    E = conn_a.shape[0]
    for bad, msg in ((c_load(1, 2, [0]), "face 2 outside 0..1"), (c_load(0, -1, [0]), "face -1 outside"),
                     (c_load(1, 1, [E]), f"element {E} outside 0..{E - 1}"), (c_load(1, 1, [-1]), "element -1 outside"),
                     (c_load(1, 1, [1, 2, 1]), "listed twice"), (c_load(2, 1, [0]), "kind must be"),
                     (c_load(1, 1, [0], (float("nan"), 0, 0)), "finite")):
        assert lib.tlfea_ancf_set_surface_loads(d._h, C.byref(bad[0]), 1) != 0 and msg in err(), msg
    arr = (tl.binding.SurfaceLoadC * 17)(*[one] * 17)
    assert lib.tlfea_ancf_set_surface_loads(d._h, arr, 17) != 0 and "0..16" in err()
    assert not d.GetLoadForces().any()
    d.SetGravity(A_G)
    k = d.AddFollowerPressure(1, [0, 1, 2, 3], 1e3)
    with pytest.raises(tl.TlfeaError, match="outside the 1 surface loads"):
        check = tl.binding.check
        check(lib.tlfea_ancf_update_load_scale(d._h, 1, 1.0))
    v = tl.SyncedVBDSolver(d, 0)
    v.SetParameters(tl.SyncedVBDParams(time_step=1e-2))
    with pytest.raises(tl.TlfeaError, match="distributed loads are set"):
        v.Solve()
    del v
    s = newton(d, 1e-2, max_inner=100)
    nl = np.zeros(d.n_coef, dtype=np.int32)
    lists = tl.binding.HaloListsC()
    ar = tl.binding.ALLREDUCE_FN(lambda u, p, n: 0)
    ex = tl.binding.HALO_EXCHANGE_FN(lambda u, sp, rp, n, pp, so, ro: 0)
    assert lib.tlfea_newton_set_halo(s._h, nl.ctypes.data_as(tl.binding.c_ip), 1, C.byref(lists), ar, ex, None, 1) != 0
    assert "distributed loads" in err()
    with pytest.raises(tl.TlfeaError, match="distributed loads"):
        s.SetInterface(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.ones(d.n_coef), lambda p, n: None)
    s.Solve()                                                            # still usable: the step of an object never refused
    got = coefs(d)
    del s
    d.Destroy()
    d = build(prob)
    d.SetGravity(A_G)
    assert d.AddFollowerPressure(1, [0, 1, 2, 3], 1e3) == k
    s = newton(d, 1e-2, max_inner=100)
    s.Solve()
    assert np.array_equal(got, coefs(d)) and np.abs(got - aonp.reference(prob)).max() > 0
    del s
    d.Destroy()
    del keep


def test_second_calc_dsdu_pre_rebuilds_the_traction_weights():
    """a second CalcDsDuPre drops the sample-point weights; the traction vector is rebuilt from the new ones, once"""
    prob = SHAPES["shell1"]()
    d = build(prob)
    d.SetGravity(A_G)
    d.AddSurfaceTraction(1, [0], T_VEC)
    s = newton(d, 1e-2)
    s.EvalGradient()
    f1 = d.GetLoadForces()
    d.CalcDsDuPre()
    d.CalcMassMatrix()
    s.EvalGradient()
    assert np.array_equal(f1, d.GetLoadForces()) and f1.any()
    L, W, H = prob[5]
    want = L * W * T_VEC + SOFT["rho0"] * L * W * H * A_G
    assert np.abs(d.GetLoadResultant() - want).max() <= 1e-12 * np.abs(want).max()
    del s
    d.Destroy()


# ---- 7. driver -------------------------------------------------------------------------------------------------------------------
def test_shell_inflation_driver():
    exe = os.path.join(HOST, "test_shell_inflation")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    p = subprocess.run(["timeout", "-k", "10", "120", exe, "--steps=6"], capture_output=True, text=True, timeout=140)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    print(p.stdout)
    ref = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("Reference:")][0]
    got, want = np.array(ref[ref.index("resultant") + 2:][:3], dtype=float), np.array(ref[ref.index("expected") + 2:][:3], dtype=float)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()         # m a - p A n at the first scale, undeformed strip
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("Step ")]
    assert len(rows) == 6
    scale = np.array([float(r[r.index("scale") + 2]) for r in rows])
    dz = np.array([float(r[r.index("dz") + 2]) for r in rows])
    assert np.all(np.diff(scale) > 0) and np.all(dz < 0) and np.all(np.diff(dz) < 0)   # deflection monotone in the ramp
