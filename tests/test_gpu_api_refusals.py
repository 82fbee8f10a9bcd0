"""The text of the refusals of the stress, obstacle and load entry points of the C-ABI, for both kinds of handle, and of the
first-order solvers: each call below is refused, and tlfea_last_error() is compared with the exact message.  The T10 and
ANCF entry points of these subsystems share their implementation, and their preconditions differ in small ways (the
tlfea_t10_* obstacle calls other than set_obstacles refuse an ANCF handle only while it holds a list; an ANCF surface load
names a face of its elements, a T10 one does not); this pins every one of them.  The meshes are the smallest at hand:
beam_3x2x1 (36 T10 elements) and the welded 20 x 20 ANCF3243 net."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import MATERIALS, load_mesh, make_gpu, tl
from tests.test_gpu_ancf_stress import SHAPES, make_ancf_gpu
from tests.test_gpu_field_obstacles import floor_box
from tests.test_gpu_obstacles import plane

pytestmark = pytest.mark.gpu
B = tl.binding
NOT_ANCF = ": T10 handles only (not an ANCF handle)"
NOT_T10 = ": ANCF handles only (not a T10 handle)"
STRESS_GETTERS = ("retrieve_point_stress", "retrieve_element_stress", "retrieve_nodal_stress", "get_energies")


@pytest.fixture()
def lib():
    return tl.load_library()


def t10_handle():
    X, conn = load_mesh("beam_3x2x1")
    return make_gpu(X, conn, MATERIALS["svk"])


def ancf_handle():
    return make_ancf_gpu(SHAPES["net"](), MATERIALS["svk"])


def refused(lib, rc, message):
    assert rc != 0
    assert lib.tlfea_last_error().decode() == message


def obstacle_list(n):
    one = plane([0.0, 0.0, -1.0], [0, 0, 1], 1e8).to_c()
    return (B.ObstacleC * max(n, 1))(*[one] * max(n, 1))


def stress_getter_args(h, name, out):
    """arguments of tlfea_<kind>_<name> with every output array set to `out` (None: null pointers)"""
    return {"retrieve_point_stress": (h, out), "retrieve_element_stress": (h, out, out, out, out, out),
            "retrieve_nodal_stress": (h, out, out), "get_energies": (h, out)}[name]


# ---- stress and energy recovery ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("t10", "ancf"))
def test_stress_refusals(lib, kind):
    own, other = (t10_handle(), ancf_handle()) if kind == "t10" else (ancf_handle(), t10_handle())
    wrong = NOT_ANCF if kind == "t10" else NOT_T10
    f = lambda name: getattr(lib, f"tlfea_{kind}_{name}")
    buf = np.zeros(8)
    vel = np.zeros(3 * other.n_coef)
    # the other kind's handle: the calc family reports under the name of calc_stress, the getters under their own
    refused(lib, f("calc_stress")(other._h, None, 0), f"tlfea_{kind}_calc_stress" + wrong)
    refused(lib, f("calc_stress_host")(other._h, None, 0), f"tlfea_{kind}_calc_stress" + wrong)
    refused(lib, f("calc_stress_host")(other._h, B.dp(vel), 0), f"tlfea_{kind}_calc_stress" + wrong)
    refused(lib, f("time_stress_kernels")(other._h, None, 0, 1, B.dp(buf)), f"tlfea_{kind}_calc_stress" + wrong)
    for name in STRESS_GETTERS:
        refused(lib, f(name)(*stress_getter_args(other._h, name, B.dp(buf))), f"tlfea_{kind}_{name}" + wrong)
    # retrieve before calc
    for name in STRESS_GETTERS:
        refused(lib, f(name)(*stress_getter_args(own._h, name, B.dp(buf))),
                f"tlfea_{kind}_{name}: tlfea_{kind}_calc_stress has not been called")
    # a null handle takes the same road
    refused(lib, f("get_energies")(None, B.dp(buf)), f"tlfea_{kind}_get_energies: tlfea_{kind}_calc_stress has not been called")
    # point stresses after a calc that did not ask for them
    assert f("calc_stress")(own._h, None, 0) == 0
    refused(lib, f("retrieve_point_stress")(own._h, B.dp(buf)),
            f"tlfea_{kind}_retrieve_point_stress: the last tlfea_{kind}_calc_stress did not ask for point stresses "
            "(want_points = 0)")
    # null outputs
    refused(lib, f("get_energies")(own._h, None), f"tlfea_{kind}_get_energies: null output")
    refused(lib, f("time_stress_kernels")(own._h, None, 0, 1, None), f"tlfea_{kind}_time_stress_kernels: null output")
    assert f("calc_stress")(own._h, None, 1) == 0
    refused(lib, f("retrieve_point_stress")(own._h, None), f"tlfea_{kind}_retrieve_point_stress: null output")
    # the element and nodal getters take null for the fields that are not wanted
    assert f("retrieve_element_stress")(own._h, None, None, None, None, None) == 0
    assert f("retrieve_nodal_stress")(own._h, None, None) == 0
    own.Destroy()
    other.Destroy()


# ---- analytic obstacles --------------------------------------------------------------------------------------------------
def test_t10_obstacle_calls_on_an_ancf_handle(lib):
    """set_obstacles and get_surface_weights refuse an ANCF handle outright; clear, update, get_forces and get_resultant
    only while the handle holds a list (which then belongs to the tlfea_ancf_* calls)"""
    a = ancf_handle()
    one, out = obstacle_list(1), np.zeros(3 * a.n_coef)
    refused(lib, lib.tlfea_t10_set_obstacles(a._h, one, 1), "tlfea_t10_set_obstacles" + NOT_ANCF)
    refused(lib, lib.tlfea_t10_get_surface_weights(a._h, B.dp(out)), "tlfea_t10_get_surface_weights" + NOT_ANCF)
    # no list: the kind is not looked at
    assert lib.tlfea_t10_clear_obstacles(a._h) == 0
    assert lib.tlfea_t10_get_obstacle_forces(a._h, B.dp(out)) == 0
    refused(lib, lib.tlfea_t10_update_obstacle(a._h, 0, one), "tlfea_t10_update_obstacle: index 0 outside the 0 obstacles set")
    refused(lib, lib.tlfea_t10_get_obstacle_resultant(a._h, 0, B.dp(out)),
            "tlfea_t10_get_obstacle_resultant: index 0 outside the 0 obstacles set")
    # a list set through the ANCF calls
    assert lib.tlfea_ancf_set_obstacles(a._h, one, 1) == 0
    refused(lib, lib.tlfea_t10_clear_obstacles(a._h), "tlfea_t10_clear_obstacles" + NOT_ANCF)
    refused(lib, lib.tlfea_t10_update_obstacle(a._h, 0, one), "tlfea_t10_update_obstacle" + NOT_ANCF)
    refused(lib, lib.tlfea_t10_get_obstacle_forces(a._h, B.dp(out)), "tlfea_t10_get_obstacle_forces" + NOT_ANCF)
    refused(lib, lib.tlfea_t10_get_obstacle_resultant(a._h, 0, B.dp(out)), "tlfea_t10_get_obstacle_resultant" + NOT_ANCF)
    a.Destroy()


def test_ancf_obstacle_calls_on_a_t10_handle(lib):
    t = t10_handle()
    one, out = obstacle_list(1), np.zeros(3 * t.n_coef)
    for name, args in (("clear_obstacles", ()), ("set_obstacles", (one, 1)), ("update_obstacle", (0, one)),
                       ("get_obstacle_forces", (B.dp(out),)), ("get_obstacle_resultant", (0, B.dp(out))),
                       ("get_surface_points", (B.dp(out),)), ("retrieve_contact_points", (B.dp(out),))):
        refused(lib, getattr(lib, f"tlfea_ancf_{name}")(t._h, *args), f"tlfea_ancf_{name}" + NOT_T10)
    t.Destroy()


@pytest.mark.parametrize("kind", ("t10", "ancf"))
def test_obstacle_argument_refusals(lib, kind):
    h = t10_handle() if kind == "t10" else ancf_handle()
    f = lambda name: getattr(lib, f"tlfea_{kind}_{name}")
    many, out = obstacle_list(17), np.zeros(3 * h.n_coef)
    # n outside 0..kMaxObstacles
    refused(lib, f("set_obstacles")(h._h, many, 17), f"tlfea_{kind}_set_obstacles: n must be in 0..16, got 17")
    refused(lib, f("set_obstacles")(h._h, many, -1), f"tlfea_{kind}_set_obstacles: n must be in 0..16, got -1")
    refused(lib, f("set_obstacles")(h._h, None, 2), f"tlfea_{kind}_set_obstacles: null list")
    # indices outside the list, null arguments
    assert f("set_obstacles")(h._h, many, 2) == 0
    for k in (2, -1):
        refused(lib, f("update_obstacle")(h._h, k, many), f"tlfea_{kind}_update_obstacle: index {k} outside the 2 obstacles set")
        refused(lib, f("get_obstacle_resultant")(h._h, k, B.dp(out)),
                f"tlfea_{kind}_get_obstacle_resultant: index {k} outside the 2 obstacles set")
    refused(lib, f("update_obstacle")(h._h, 1, None), f"tlfea_{kind}_update_obstacle: null obstacle")
    refused(lib, f("get_obstacle_resultant")(h._h, 1, None), f"tlfea_{kind}_get_obstacle_resultant: null output")
    refused(lib, f("get_obstacle_forces")(h._h, None), f"tlfea_{kind}_get_obstacle_forces: null output")
    if kind == "t10":
        refused(lib, lib.tlfea_t10_get_surface_weights(h._h, None), "tlfea_t10_get_surface_weights: null output")
    else:
        refused(lib, lib.tlfea_ancf_get_surface_points(h._h, None), "tlfea_ancf_get_surface_points: null output")
        refused(lib, lib.tlfea_ancf_retrieve_contact_points(h._h, None), "tlfea_ancf_retrieve_contact_points: null output")
    # a bad obstacle is named by its index
    bad = obstacle_list(2)
    bad[1].stiffness = 0.0
    assert f("set_obstacles")(h._h, bad, 2) != 0
    assert lib.tlfea_last_error().decode().startswith(f"tlfea_{kind}_set_obstacles: obstacle 1: ")
    assert f("update_obstacle")(h._h, 0, C.byref(bad[1])) != 0
    assert lib.tlfea_last_error().decode().startswith(f"tlfea_{kind}_update_obstacle: obstacle 0: ")
    # analytic and field obstacles together
    assert f("clear_obstacles")(h._h) == 0
    h.SetFieldObstacles([floor_box(-1.0, 1e8)] * 6)
    refused(lib, f("set_obstacles")(h._h, many, 11),
            f"tlfea_{kind}_set_obstacles: 11 analytic and 6 field obstacles exceed the 16 an object can hold")
    assert f("set_obstacles")(h._h, many, 10) == 0
    h.Destroy()


# ---- distributed loads ---------------------------------------------------------------------------------------------------
def test_load_calls_on_the_other_kind(lib):
    t, a = t10_handle(), ancf_handle()
    buf = np.zeros(8, dtype=np.int32)
    refused(lib, lib.tlfea_t10_get_boundary_faces(a._h, B.ip(buf), None, None, None), "tlfea_t10_get_boundary_faces" + NOT_ANCF)
    refused(lib, lib.tlfea_t10_set_surface_loads(a._h, None, 0), "tlfea_t10_set_surface_loads" + NOT_ANCF)
    refused(lib, lib.tlfea_t10_update_load_scale(a._h, 0, 1.0), "tlfea_t10_update_load_scale" + NOT_ANCF)
    refused(lib, lib.tlfea_ancf_set_surface_loads(t._h, None, 0),
            "tlfea_ancf_set_surface_loads: ANCF handles only (a T10 handle takes the body acceleration alone)")
    refused(lib, lib.tlfea_ancf_update_load_scale(t._h, 0, 1.0), "tlfea_ancf_update_load_scale" + NOT_T10)
    t.Destroy()
    a.Destroy()


def load_array(kind, entries):
    """the ctypes list of tlfea_<kind>_set_surface_loads from (load kind, face, value[3], scale, indices) entries, and the
    index arrays it points into (to be kept alive during the call); an empty index list travels as a null pointer"""
    keep = [np.asarray(e[4], dtype=np.int32) for e in entries]
    ptr = lambda a: B.ip(a) if a.size else None
    if kind == "t10":
        items = [B.T10SurfaceLoadC(k, tuple(v), sc, ptr(a), int(a.size)) for (k, _, v, sc, _), a in zip(entries, keep)]
        return (B.T10SurfaceLoadC * len(items))(*items), keep
    items = [B.SurfaceLoadC(k, f, tuple(v), sc, ptr(a), int(a.size)) for (k, f, v, sc, _), a in zip(entries, keep)]
    return (B.SurfaceLoadC * len(items))(*items), keep


@pytest.mark.parametrize("kind", ("t10", "ancf"))
def test_surface_load_refusals(lib, kind):
    """every refusal of set_surface_loads and update_load_scale, in the order the checks run; a refused call leaves the
    load of the last gradient evaluation (tlfea_get_load_resultant) and the stored list (the load of the next gradient
    evaluation) as they were, and a valid list is still taken after it"""
    h = t10_handle() if kind == "t10" else ancf_handle()
    P, U = f"tlfea_{kind}_set_surface_loads", f"tlfea_{kind}_update_load_scale"
    set_loads, update = getattr(lib, P), getattr(lib, U)
    if kind == "t10":
        n = C.c_int()
        assert lib.tlfea_t10_get_boundary_faces(h._h, C.byref(n), None, None, None) == 0
        R, noun = n.value, "face"
    else:
        R, noun = h.get_n_elem(), "element"
    v, nan = (0.0, 0.0, -1e3), float("nan")
    good = [(0, 1, v, 1.0, [0, 1, 2]), (1, 1, (2e3, 0.0, 0.0), 0.5, [1, 2])]
    good_arr, good_keep = load_array(kind, good)

    def resultant():
        out = np.zeros(3)
        assert lib.tlfea_get_load_resultant(h._h, B.dp(out)) == 0
        return out

    assert set_loads(h._h, good_arr, 2) == 0
    s = tl.SyncedNewtonSolver(h, 0)
    s.EvalGradient()
    R0 = resultant()
    assert np.linalg.norm(R0) > 0.0

    def after_refusal():
        assert np.array_equal(resultant(), R0)      # the buffers of the last evaluation were not touched ...
        s.EvalGradient()                            # ... and the list the handle holds is still the one that was set:
        assert np.allclose(resultant(), R0, rtol=1e-12, atol=1e-12 * np.max(np.abs(R0)))  # the same sums, to rounding
        assert set_loads(h._h, good_arr, 2) == 0

    # the count and the list pointer
    for n in (-1, 17):
        refused(lib, set_loads(h._h, good_arr, n), f"{P}: n must be in 0..16, got {n}")
        after_refusal()
    refused(lib, set_loads(h._h, None, 2), f"{P}: null list")
    after_refusal()
    # one bad load behind a good one: named by its index
    cases = [((2, 1, v, 1.0, [0]), "kind must be 0 (traction) or 1 (pressure), got 2"),
             ((-1, 1, v, 1.0, [0]), "kind must be 0 (traction) or 1 (pressure), got -1"),
             ((0, 1, (0.0, 0.0, nan), 1.0, [0]), "the value must be finite"),
             ((1, 1, (nan, 0.0, 0.0), 1.0, [0]), "the value must be finite"),
             ((0, 1, v, nan, [0]), "the scale must be finite"),
             ((0, 1, v, 1.0, []), f"empty {noun} list"),
             ((0, 1, v, 1.0, [0, -1]), f"{noun} -1 outside 0..{R - 1}"),
             ((0, 1, v, 1.0, [0, R]), f"{noun} {R} outside 0..{R - 1}"),
             ((0, 1, v, 1.0, [3, 0, 3]), f"{noun} 3 is listed twice" + (" for face 1" if kind == "ancf" else ""))]
    if kind == "ancf":  # the 3243 beam has faces 0..3; the face is looked at before the value
        cases += [((0, -1, v, 1.0, [0]), "face -1 outside 0..3"), ((0, 4, (nan, 0.0, 0.0), 1.0, [0]), "face 4 outside 0..3")]
    for bad, text in cases:
        arr, keep = load_array(kind, [good[0], bad])
        refused(lib, set_loads(h._h, arr, 2), f"{P}: load 1: {text}")
        after_refusal()
    # the scale update
    for k in (2, -1):
        refused(lib, update(h._h, k, 1.0), f"{U}: index {k} outside the 2 surface loads set")
        after_refusal()
    refused(lib, update(h._h, 0, nan), f"{U}: the scale must be finite")
    after_refusal()
    # the list is the one that was set: the same load again (sums of the same terms: to rounding of their order at most)
    s.EvalGradient()
    assert np.allclose(resultant(), R0, rtol=1e-12, atol=1e-12 * np.max(np.abs(R0)))
    del s, good_keep
    h.Destroy()


# ---- first-order solvers -------------------------------------------------------------------------------------------------
FIRST_ORDER = {"adamw": ("SyncedAdamWNocoopSolver", "SyncedAdamWNocoop"), "nesterov": ("SyncedNesterovSolver", "SyncedNesterov"),
               "vbd": ("SyncedVBDSolver", "SyncedVBDSolver")}


def test_first_order_create_and_parameter_refusals(lib):
    t = t10_handle()
    out = C.c_void_p()
    for name, (cls, _) in FIRST_ORDER.items():
        create = getattr(lib, f"tlfea_{name}_create")
        refused(lib, create(None, 0, C.byref(out)), f"tlfea_{name}_create: null argument")
        refused(lib, create(t._h, 0, None), f"tlfea_{name}_create: null argument")
        s = getattr(tl, cls)(t, 0)
        refused(lib, getattr(lib, f"tlfea_{name}_set_parameters")(s._h, None), "null argument")
        del s
    t.Destroy()


def test_first_order_solve_refusals(lib):
    # AdamW and Nesterov before CalcMassMatrix: the gradient needs the mass pattern
    a = make_ancf_gpu(SHAPES["net"](), MATERIALS["svk"], mass=False)
    for name in ("adamw", "nesterov"):
        cls, who = FIRST_ORDER[name]
        s = getattr(tl, cls)(a, 0)
        refused(lib, getattr(lib, f"tlfea_{name}_solve")(s._h),
                f"{who}: CalcMassMatrix() must precede Solve() (the gradient uses the mass CSR)")
        del s
    a.Destroy()
    # Nesterov with general linear constraints (cons_mode 2): the pinned DOFs of the beam's end face as CSR rows
    X, conn = load_mesh("beam_3x2x1")
    m, q = MATERIALS["svk"], tl.quadrature
    d = tl.GPU_FEAT10_Data(conn.shape[0], X.shape[0])
    d.Initialize()
    d.Setup(q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights, X[:, 0], X[:, 1], X[:, 2], conn)
    d.SetDensity(m["rho0"])
    d.SetDamping(m["eta"], m["lamd"])
    d.SetSVK(m["E"], m["nu"])
    fx = np.where(np.abs(X[:, 0]) < 1e-8)[0]
    cols = (3 * fx[:, None] + np.arange(3)[None, :]).reshape(-1)
    d.SetLinearConstraintsCSR(np.arange(len(cols) + 1), cols, np.ones(len(cols)), X[fx].reshape(-1))
    d.CalcDnDuPre()
    d.CalcMassMatrix()
    d.CalcConstraintData()
    assert d.GetConstraintMode() == 2
    s = tl.SyncedNesterovSolver(d, d.get_n_constraint())
    refused(lib, lib.tlfea_nesterov_solve(s._h), "SyncedNesterov: fixed-coefficient constraints only (as the reference, :197-200)")
    del s
    d.Destroy()
    # VBD has neither a contact nor a load term: an obstacle is looked at first, then the loads
    t = t10_handle()
    s = tl.SyncedVBDSolver(t, 0)
    assert lib.tlfea_t10_set_obstacles(t._h, obstacle_list(1), 1) == 0
    g = np.array([0.0, 0.0, -9.81])
    assert lib.tlfea_set_body_acceleration(t._h, B.dp(g)) == 0
    refused(lib, lib.tlfea_vbd_solve(s._h),
            "SyncedVBDSolver: rigid obstacles are set, and the VBD vertex solve has no contact term; use the Newton, AdamW or "
            "Nesterov solver, or clear the obstacles")
    assert lib.tlfea_t10_clear_obstacles(t._h) == 0
    refused(lib, lib.tlfea_vbd_solve(s._h),
            "SyncedVBDSolver: distributed loads are set, and the VBD vertex solve has no load term; use the Newton, AdamW or "
            "Nesterov solver, or clear the loads")
    del s
    t.Destroy()
