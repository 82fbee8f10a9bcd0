"""Surface loads on T10 boundary faces on the GPU (DESIGN 3h'): dead traction and follower pressure against
tests/t10_loads_np.py (pinned without a GPU by tests/test_t10_loads_np.py).  Kernel parity, bitwise checks, the hydrostatic
state, a traction step against the same vector through SetExternalForce, the fixed point of a follower-pressure step,
Nesterov, the refusals and the driver.  Shapes: one tet (every node on the surface), the 1 x 1 x 1 and 2 x 3 x 1 boxes,
beam_3x2x1, sphere.1 (curved faces, more than one block of loaded faces) and the 1 x 1 x 1 box with displaced mid-edge
nodes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import t10_loads_np as lnp
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_gpu, make_oracle, tl
from tests.test_t10_loads_np import LAM, hydrostatic_pressure, sphere

pytestmark = pytest.mark.gpu
mu = tl.mesh_utils
EPS = np.finfo(float).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
SVK = MATERIALS["svk"]
SOFT = dict(kind="svk", E=1e6, nu=0.3, rho0=1000.0, eta=0.0, lamd=0.0)
A_G = np.array([0.3, -0.2, -9.81])
T_VEC = np.array([120.0, -80.0, 300.0])
SHAPE_NAMES = ("tet1", "box111", "box231", "beam_3x2x1", "sphere", "box111_curved")


@functools.lru_cache(maxsize=None)
def shape(name):
    """(X, conn) of a test shape: shared, never modified"""
    if name == "tet1":
        V = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.2, 0.8]])
        X = np.concatenate([V, [0.5 * (V[a] + V[b]) for a, b in mu.EDGES]])
        return X, np.arange(10, dtype=np.int32)[None, :]
    if name == "box111":
        return mu.structured_t10_box(1, 1, 1)
    if name == "box231":
        return mu.structured_t10_box(2, 3, 1, 1.5, 1.0, 0.8)
    if name == "sphere":
        return sphere()
    if name == "box111_curved":
        X, conn = mu.structured_t10_box(1, 1, 1)
        mids = np.unique(lnp.boundary_faces(X, conn)[2][:, 3:])
        X = X.copy()
        X[mids] += np.random.default_rng(5).normal(0, 0.02, (len(mids), 3))
        return X, conn
    return load_mesh(name)


@functools.lru_cache(maxsize=None)
def scene(name):
    """perturbed positions, the boundary faces and the load sets of the parity test: each kind alone, gravity with a
    traction and two pressures that overlap on some faces, and a subset that leaves nodes with loaded and unloaded
    incident faces"""
    X, conn = shape(name)
    x = X + np.random.default_rng(11).normal(0, 2e-3 * np.abs(X).max(), X.shape)
    elem, lf, nodes = lnp.boundary_faces(X, conn)
    faces = np.arange(len(elem))
    trac = [dict(kind=0, faces=faces, value=T_VEC, scale=1.5), dict(kind=0, faces=faces[::2], value=-0.5 * T_VEC, scale=1.0)]
    press = [dict(kind=1, faces=faces, value=3e4, scale=0.75), dict(kind=1, faces=faces[:1], value=-1.2e4, scale=1.0),
             dict(kind=1, faces=faces[::2], value=5e3, scale=2.0)]
    part = [dict(kind=0, faces=faces[::3], value=T_VEC, scale=1.0), dict(kind=1, faces=faces[1::3], value=3e4, scale=1.0)]
    sets = {"traction": (None, trac[:1]), "pressure": (None, press[:1]), "all": (A_G, trac + press), "subset": (None, part)}
    return X, conn, x, (elem, lf, nodes), sets


@functools.lru_cache(maxsize=None)
def gravity_force(name):
    """M a with the oracle's mass matrix (tests/test_gpu_ancf_loads.py::test_t10_gravity pins the kernel against it)"""
    X, conn = shape(name)
    o = make_oracle(X, conn, SVK)
    f = np.zeros((X.shape[0], 3))
    for i in range(X.shape[0]):
        f[i] = o.m_val[o.m_off[i]:o.m_off[i + 1]].sum() * A_G
    return f


def reference(name, which, scales=None):
    X, conn, x, (_, _, nodes), sets = scene(name)
    g, loads = sets[which]
    if scales is not None:
        loads = [dict(ld, scale=s) for ld, s in zip(loads, scales)]
    return lnp.total(X, x, nodes, loads, gravity_force(name) if g is not None else None)


def apply(d, gravity, loads):
    if gravity is not None:
        d.SetGravity(gravity)
    for ld in loads:
        (d.AddFaceTraction if ld["kind"] == 0 else d.AddFacePressure)(ld["faces"], ld["value"], ld["scale"])


def newton(d, h, atol=1e-7, max_inner=40, method=0, rho=1e14):
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(atol, 0.0, 1e-6, rho, 1, max_inner, h))
    s.SetLinSolveOpts(tl.LinSolveOpts(rel_tol=1e-13, max_iter=50000, method=method))
    return s


def move(d, x):
    d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])


def coords(d):
    return np.stack(d.RetrievePositionToCPU(), axis=1)


def close_positions(xa, xb, x0):
    """the project's rule for two runs of one step: 1e-10 of the displacement + 8 ulp of the coordinates"""
    disp = np.abs(xa - x0).max()
    err = np.abs(xa - xb).max()
    print(f"  displacement {disp:.3e}  difference {err:.3e}")
    return err <= 1e-10 * disp + 8 * EPS * np.abs(x0).max()


# ---- 1. boundary faces, parity with the restatement, two evaluations, the resultant, a scale change -------------------------
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_kernel_parity(name):
    """Parity bound: 1e-13 of the largest row (the bound of tests/test_gpu_ancf_loads.py).  Measured on the MI355X, largest
    over the load sets: force 3.8e-16 .. 7.7e-16, gradient 3.9e-17 .. 9.2e-17 (DESIGN 3h')."""
    X, conn, x, (elem, lf, nodes), sets = scene(name)
    d = make_gpu(X, conn, SVK)
    bf = d.GetBoundaryFaces()
    assert np.array_equal(bf.elem, elem) and np.array_equal(bf.local_face, lf) and np.array_equal(bf.nodes, nodes)
    cen, nrm, area = lnp.face_geometry(X, nodes)
    assert np.array_equal(bf.centroid, cen) and np.array_equal(bf.normal, nrm) and np.array_equal(bf.area, area)
    s = newton(d, 1e-2)
    move(d, x)
    s.BeginStep()
    s.EvalGradient()
    g0 = s.RetrieveGradientToCPU()
    assert not d.GetLoadForces().any()

    def check(which, scales=None):
        s.EvalGradient()
        f, g1 = d.GetLoadForces(), s.RetrieveGradientToCPU()
        s.EvalGradient()
        assert np.array_equal(f, d.GetLoadForces()) and np.array_equal(g1, s.RetrieveGradientToCPU())   # bitwise
        ref = reference(name, which, scales)
        scale = np.abs(ref).max()
        err = np.abs(f.reshape(-1, 3) - ref).max() / scale
        err_g = np.abs((g1 - g0) + f).max() / max(scale, np.abs(g0).max())
        print(name, which, scales, f"force {err:.2e}  gradient {err_g:.2e}")
        assert err <= 1e-13
        assert err_g <= 1e-13
        assert np.abs(d.GetLoadResultant() - f.reshape(-1, 3).sum(axis=0)).max() <= 1e-12 * np.abs(f).sum()

    for which, (g, loads) in sets.items():
        apply(d, g, loads)
        check(which)
        if which == "all":                                               # ramp a traction and a pressure, send nothing again
            scales = [ld["scale"] for ld in loads]
            scales[0], scales[2] = 0.25, -1.5
            d.SetFaceLoadScale(0, scales[0])
            d.SetFaceLoadScale(2, scales[2])
            check(which, tuple(scales))
        d.ClearLoads()
        s.EvalGradient()
        assert not d.GetLoadForces().any() and np.array_equal(s.RetrieveGradientToCPU(), g0)
    del s
    d.Destroy()


# ---- 2. the hydrostatic state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["beam_3x2x1", "sphere"])
def test_hydrostatic_state(name):
    """x = lam X, v = 0, no constraints, the pressure that holds it on every boundary face: the gradient f_int - f_load
    vanishes within 1e-12 of the largest internal-force row, the bound of tests/test_t10_loads_np.py.  Measured on the
    MI355X: 3.9e-14 (beam_3x2x1, |g|_2 = 1.9e-6) and 1.0e-13 (sphere.1, |g|_2 = 3.2e-8)."""
    X, conn = shape(name)
    d = make_gpu(X, conn, SVK)
    n_faces = len(d.GetBoundaryFaces().elem)
    d.AddFacePressure(np.arange(n_faces), hydrostatic_pressure(SVK))
    s = newton(d, 1e-2)
    move(d, LAM * X)
    s.BeginStep()
    s.EvalGradient()
    g = s.RetrieveGradientToCPU()
    fint = d.RetrieveInternalForceToCPU()
    scale = np.abs(fint).max()
    print(name, f"|g|_max {np.abs(g).max():.3e}  |g|_2 {np.linalg.norm(g):.3e}  largest internal-force row {scale:.3e}"
          f"  ratio {np.abs(g).max() / scale:.2e}")
    assert scale > 0 and np.abs(g).max() <= 1e-12 * scale
    del s
    d.Destroy()


# ---- 3. a traction in a step: the same vector through SetExternalForce -----------------------------------------------------------
def end_faces(d):
    bf = d.GetBoundaryFaces()
    return np.nonzero(bf.normal[:, 0] > 0.99)[0]


# The internal force of this material is rounded at about E EPS per stress, 7e8 x 2.2e-16 x a few, times the weights of a
# hundred points per row: |g|_2 cannot fall below 1e-6 .. 1e-5 on these meshes (test_hydrostatic_state prints 1.9e-6).  The
# steps below iterate to 1e-4, which is 1e-9 of the traction's rows (t A_face / 3 ~ 1e5) and 1e-7 of the refusal test's.
ATOL_STEP = 1e-4


@pytest.mark.parametrize("method", [0, 1])
def test_traction_step_like_external_force(method):
    X, conn = shape("beam_3x2x1")
    fixed = fixed_x0(X)
    t = 1e3 * T_VEC
    d = make_gpu(X, conn, SVK, fixed)
    d.AddFaceTraction(end_faces(d), t)
    s = newton(d, 1e-2, atol=ATOL_STEP, method=method, rho=1e10)
    s.EvalGradient()
    vec = d.GetLoadForces()                                               # the vector test_kernel_parity pins
    assert vec.any() and not d.RetrieveExternalForceToCPU().any()        # beside f_ext, not in it
    del s
    d.Destroy()
    out = {}
    for how in ("loads", "f_ext"):
        d = make_gpu(X, conn, SVK, fixed, None if how == "loads" else vec)
        if how == "loads":
            d.AddFaceTraction(end_faces(d), t)
        s = newton(d, 1e-2, atol=ATOL_STEP, method=method, rho=1e10)
        counts = []
        for _ in range(3):
            s.Solve()
            counts.append(s.GetStats()["newton"])
        out[how] = (coords(d), counts)
        del s
        d.Destroy()
    print(method, out["loads"][1], out["f_ext"][1])
    assert out["loads"][1] == out["f_ext"][1] and max(out["loads"][1]) < 40
    assert close_positions(out["loads"][0], out["f_ext"][0], X)


def test_nesterov_takes_the_traction_through_the_same_evaluation():
    X, conn = shape("box231")
    _, _, nodes = lnp.boundary_faces(X, conn)
    faces = np.arange(len(nodes))[::2]
    vec = lnp.traction_force(X, nodes, faces, 1e3 * T_VEC).reshape(-1)
    out = {}
    for how in ("loads", "f_ext"):
        d = make_gpu(X, conn, SVK, None, None if how == "loads" else vec)
        if how == "loads":
            d.AddFaceTraction(faces, 1e3 * T_VEC)
        s = tl.SyncedNesterovSolver(d, 0)
        s.SetParameters(tl.SyncedNesterovParams(max_outer=1, max_inner=20, time_step=1e-3))
        s.Setup()
        s.Solve()
        out[how] = coords(d)
        del s
        d.Destroy()
    assert np.abs(out["loads"] - X).max() > 0
    assert close_positions(out["loads"], out["f_ext"], X)


# ---- 4. follower pressure in a step: fixed-point consistency ---------------------------------------------------------------------
def test_follower_pressure_step_is_a_fixed_point():
    """The rule of DESIGN 3h: H lacks the load stiffness, so Newton converges linearly in the pressure term; both runs are
    iterated to the floor (an inner tolerance below it, a fixed count well past convergence) and compared by the position
    rule.  The floor of |g|: the internal force is rounded at K EPS |x| with K ~ E L summed over a node's elements, about
    1e6 x 2.2e-16 x 3 x 50 = 3e-8 for the soft material here; the clamp's penalty h rho c at 1e-2 x 1e8 x 2.2e-16 x 3 =
    7e-10.  Asserted: |g| <= 1e-8 of the largest load row (333 N on this mesh, so 3.3e-6), on both runs.  Measured on the
    MI355X: |g| = 3.1e-9 and 2.9e-9; the two steps end 4.4e-16 apart at a displacement of 3.5e-4."""
    X, conn = shape("beam_3x2x1")
    fixed = fixed_x0(X)
    h, p, rho, n_fix = 1e-2, 1e3, 1e8, 30
    d = make_gpu(X, conn, SOFT, fixed)
    top = np.nonzero(d.GetBoundaryFaces().normal[:, 2] > 0.99)[0]
    _, _, nodes = lnp.boundary_faces(X, conn)
    floor = 1e-8 * np.abs(lnp.pressure_force(X, nodes, top, p)).max()
    d.AddFacePressure(top, p)
    s = newton(d, h, atol=1e-13, max_inner=n_fix, rho=rho)
    s.Solve()
    st = s.GetStats()
    print("to the floor, follower pressure:", st, "bound", floor)
    assert st["norm_g"] <= floor
    xs, fs = coords(d), d.GetLoadForces()
    ref = lnp.pressure_force(xs, nodes, top, p)
    assert np.abs(fs.reshape(-1, 3) - ref).max() <= 1e-13 * np.abs(ref).max()    # the load of the converged positions
    del s
    d.Destroy()
    d = make_gpu(X, conn, SOFT, fixed, fs)
    s = newton(d, h, atol=1e-13, max_inner=n_fix, rho=rho)
    s.Solve()
    st2 = s.GetStats()
    print("to the floor, f* as f_ext:", st2)
    assert st2["norm_g"] <= floor
    assert close_positions(xs, coords(d), X)
    del s
    d.Destroy()
    tip = np.where(np.abs(X[:, 0] - X[:, 0].max()) < 1e-12)[0]
    assert np.all(xs[tip, 2] - X[tip, 2] < 0)                                     # top face, normal +z: pushed toward -z


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def c_load(kind, faces, value=(1e3, 0.0, 0.0), scale=1.0):
    f = np.ascontiguousarray(faces, dtype=np.int32)
    return tl.binding.T10SurfaceLoadC(kind, tuple(value), scale, tl.binding.ip(f), int(f.size)), f


def test_refusals_leave_the_object_usable():
    lib = tl.load_library()
    err = lambda: lib.tlfea_last_error().decode()
    X, conn = shape("box111")
    q = tl.quadrature
    one, keep = c_load(1, [0, 1])
    n = C.c_int()
    # before Setup; then the same object is set up and steps
    d = tl.GPU_FEAT10_Data(conn.shape[0], X.shape[0])
    d.Initialize()
    assert lib.tlfea_t10_set_surface_loads(d._h, C.byref(one), 1) != 0 and "set up" in err()
    assert lib.tlfea_t10_get_boundary_faces(d._h, C.byref(n), None, None, None) != 0 and "set up" in err()
    assert lib.tlfea_t10_update_load_scale(d._h, 0, 1.0) != 0 and "set up" in err()
    d.Setup(q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights, X[:, 0], X[:, 1], X[:, 2], conn)
    d.SetDensity(SVK["rho0"])
    d.SetDamping(0.0, 0.0)
    d.SetSVK(SVK["E"], SVK["nu"])
    d.CalcDnDuPre()
    d.CalcMassMatrix()
    s = newton(d, 1e-3, atol=ATOL_STEP)

    def step():
        s.Solve()
        st = s.GetStats()
        assert np.isfinite(coords(d)).all() and st["norm_g"] <= ATOL_STEP and st["newton"] < 40, st

    step()
    assert lib.tlfea_t10_get_boundary_faces(d._h, C.byref(n), None, None, None) == 0 and n.value == 12
    F = n.value
    # the ANCF entry points keep refusing a T10 handle
    anc = tl.binding.SurfaceLoadC(1, 1, (1e3, 0.0, 0.0), 1.0, tl.binding.ip(keep), 2)
    assert lib.tlfea_ancf_set_surface_loads(d._h, C.byref(anc), 1) != 0 and "ANCF handles only" in err()
    step()
    assert lib.tlfea_ancf_update_load_scale(d._h, 0, 1.0) != 0 and "ANCF handles only" in err()
    step()
    # the list checks of the C-ABI (the mirror refuses the same earlier: tests/test_t10_loads_np.py)
    for bad, msg in ((c_load(1, [F]), f"face {F} outside 0..{F - 1}"), (c_load(0, [-1]), "face -1 outside"),
                     (c_load(1, [1, 2, 1]), "listed twice"), (c_load(2, [0]), "kind must be"),
                     (c_load(-1, [0]), "kind must be"), (c_load(1, [0], (float("nan"), 0, 0)), "finite"),
                     (c_load(0, [0], (0.0, 0.0, float("inf"))), "finite"), (c_load(1, [0], scale=float("nan")), "finite"),
                     (c_load(1, []), "empty face list")):
        assert lib.tlfea_t10_set_surface_loads(d._h, C.byref(bad[0]), 1) != 0 and msg in err(), msg
        assert not d.GetLoadForces().any()
        step()
    arr = (tl.binding.T10SurfaceLoadC * 17)(*[one] * 17)
    assert lib.tlfea_t10_set_surface_loads(d._h, arr, 17) != 0 and "0..16" in err()
    step()
    assert lib.tlfea_t10_update_load_scale(d._h, 0, 1.0) != 0 and "outside the 0 surface loads" in err()
    step()
    d.SetGravity(A_G)
    k = d.AddFacePressure(np.arange(F), 1e3)
    assert lib.tlfea_t10_update_load_scale(d._h, 1, 1.0) != 0 and "outside the 1 surface loads" in err()
    step()
    assert lib.tlfea_t10_update_load_scale(d._h, -1, 1.0) != 0 and "outside the 1 surface loads" in err()
    assert lib.tlfea_t10_update_load_scale(d._h, 0, float("inf")) != 0 and "finite" in err()
    step()
    # the solvers that have no load term
    v = tl.SyncedVBDSolver(d, 0)
    v.SetParameters(tl.SyncedVBDParams(time_step=1e-3))
    with pytest.raises(tl.TlfeaError, match="distributed loads are set"):
        v.Solve()
    del v
    step()
    nl = np.zeros(d.n_coef, dtype=np.int32)
    lists = tl.binding.HaloListsC()
    ar = tl.binding.ALLREDUCE_FN(lambda u, p, n: 0)
    ex = tl.binding.HALO_EXCHANGE_FN(lambda u, sp, rp, n, pp, so, ro: 0)
    assert lib.tlfea_newton_set_halo(s._h, nl.ctypes.data_as(tl.binding.c_ip), 1, C.byref(lists), ar, ex, None, 1) != 0
    assert "distributed loads" in err()
    step()
    with pytest.raises(tl.TlfeaError, match="distributed loads"):
        s.SetInterface(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.ones(d.n_coef), lambda p, n: None)
    step()
    assert d.GetLoadForces().any() and k == 0
    d.ClearLoads()                                                       # removes the face loads and the gravity
    s.EvalGradient()
    assert not d.GetLoadForces().any()
    del s
    d.Destroy()
    # the new entry points on an ANCF handle
    from tests.test_gpu_ancf_loads import SHAPES, build as ancf_build, newton as ancf_newton
    a = ancf_build(SHAPES["shell1"]())
    assert lib.tlfea_t10_set_surface_loads(a._h, C.byref(one), 1) != 0 and "T10 handles only" in err()
    assert lib.tlfea_t10_update_load_scale(a._h, 0, 1.0) != 0 and "T10 handles only" in err()
    assert lib.tlfea_t10_get_boundary_faces(a._h, C.byref(n), None, None, None) != 0 and "T10 handles only" in err()
    sa = ancf_newton(a, 1e-2)
    sa.Solve()
    assert np.isfinite(np.stack(a.RetrievePositionToCPU())).all()
    del sa
    a.Destroy()
    del keep


# ---- 6. driver -------------------------------------------------------------------------------------------------------------------
def test_pressurized_block_driver():
    exe = os.path.join(HOST, "test_pressurized_block")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    p = subprocess.run(["timeout", "-k", "10", "120", exe, "--steps=4"], capture_output=True, text=True, timeout=140)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    print(p.stdout)
    ref = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("Reference:")][0]
    got, want = np.array(ref[ref.index("resultant") + 2:][:3], dtype=float), np.array(ref[ref.index("expected") + 2:][:3], dtype=float)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()         # m a - p A n at the first scale, undeformed block
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("Step ")]
    assert len(rows) == 4
    scale = np.array([float(r[r.index("scale") + 2]) for r in rows])
    dz = np.array([float(r[r.index("dz") + 2]) for r in rows])
    assert np.all(np.diff(scale) > 0) and np.all(dz < 0) and np.all(np.diff(dz) < 0)   # pushed further down as the ramp rises
