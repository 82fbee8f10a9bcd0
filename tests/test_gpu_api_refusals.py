"""The text of the refusals of the stress, obstacle and load entry points of the C-ABI, for both kinds of handle: each
call below is refused, and tlfea_last_error() is compared with the exact message.  The T10 and ANCF entry points of these
subsystems share their implementation, and their preconditions differ in small ways (the tlfea_t10_* obstacle calls other
than set_obstacles refuse an ANCF handle only while it holds a list); this pins every one of them.  The meshes are the
smallest at hand: beam_3x2x1 (36 T10 elements) and the welded 20 x 20 ANCF3243 net."""
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
