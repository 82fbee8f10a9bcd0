"""Rigid obstacles without a GPU: the NumPy model against finite differences (gradient and block, both kinds, both
friction branches), PSD friction blocks, surface weights against exact areas, the exported symbols, the Python layer's
refusals before any ABI call, and the build of the rigid-floor driver."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import obstacles_np as onp
from tests.helpers import load_mesh

tl = importlib.import_module("total-lagrangian-fea_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
NEW = ("tlfea_t10_set_obstacles", "tlfea_t10_update_obstacle", "tlfea_t10_clear_obstacles",
       "tlfea_t10_get_obstacle_forces", "tlfea_t10_get_obstacle_resultant", "tlfea_t10_get_surface_weights")

H = 1e-2
PLANE = dict(kind=0, p=np.array([0.1, -0.2, 0.3]), n=np.array([1.0, 2.0, 2.0]) / 3.0, kappa=3e5, mu=0.4,
             eps_v=1e-2, vel=np.array([0.05, -0.02, 0.01]))
SPHERE = dict(kind=1, p=np.array([0.0, 0.0, -1.0]), radius=1.2, kappa=2e5, mu=0.3, eps_v=1e-2,
              vel=np.array([-0.01, 0.03, 0.0]))


def _state(o, slip, rng):
    """A node in contact at the start of the step and now, with a tangential slip of about `slip` (x eps_v h)."""
    if o["kind"] == 0:
        q0 = o["p"] + rng.normal(0, 0.1, 3)
        q0 -= (o["n"] @ (q0 - o["p"]) + 2e-3) * o["n"]
        n = o["n"]
    else:
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        q0 = o["p"] + (o["radius"] - 2e-3) * n
    t = np.cross(n, rng.normal(size=3))
    t /= np.linalg.norm(t)
    q = q0 + H * o["vel"] + slip * o["eps_v"] * H * t - 5e-4 * n + rng.normal(0, 1e-6, 3)
    return q, q0


@pytest.mark.parametrize("o", [PLANE, SPHERE], ids=["plane", "sphere"])
@pytest.mark.parametrize("slip", [0.3, 3.0], ids=["stick", "slide"])
def test_gradient_and_block_match_finite_differences(o, slip):
    rng = np.random.default_rng(7)
    w = 0.37
    for _ in range(5):
        q, q0 = _state(o, slip, rng)
        f, B = onp.force_block(o, w, q, q0, H)
        e = 1e-7
        g_fd = np.array([(onp.energy(o, w, q + e * u, q0, H) - onp.energy(o, w, q - e * u, q0, H)) / (2 * e)
                         for u in np.eye(3)])
        assert np.allclose(-f, g_fd, rtol=1e-6, atol=1e-6 * np.abs(f).max())
        J = np.array([-(onp.force_block(o, w, q + e * u, q0, H)[0] - onp.force_block(o, w, q - e * u, q0, H)[0]) / (2 * e)
                      for u in np.eye(3)]).T
        if o["kind"] == 1:
            # Gauss-Newton: the engine drops the curvature term kappa w d / r (I - n n^T) of the sphere (negative in contact)
            d, n = onp.distance(o, q)
            J -= o["kappa"] * w * d / (d + o["radius"]) * (np.eye(3) - np.outer(n, n))
        assert np.allclose(J, J.T, atol=1e-4 * np.abs(B).max())
        assert np.allclose(B, J, rtol=1e-5, atol=1e-5 * np.abs(B).max())


def test_friction_block_is_psd():
    rng = np.random.default_rng(11)
    for o in (PLANE, SPHERE):
        for _ in range(200):
            q, q0 = _state(o, float(rng.uniform(0, 4)), rng)
            _, B = onp.force_block(o, float(rng.uniform(0.01, 1)), q, q0, H)
            assert np.allclose(B, B.T)
            assert np.linalg.eigvalsh(B).min() >= -1e-9 * np.abs(B).max()


def test_surface_weights_sum_to_area():
    for X, conn, area in ((*load_mesh("beam_3x2x1"), 2 * (3 * 2 + 3 * 1 + 2 * 1)), (*load_mesh("cube"), 6.0),
                          (*tl.mesh_utils.structured_t10_box(3, 2, 2, 1.5, 1.0, 0.8), 2 * (1.5 + 1.2 + 0.8))):
        w = onp.surface_weights(X, conn)
        assert abs(w.sum() - area) < 1e-12 * area
        lo, hi = X.min(0), X.max(0)
        interior = np.all((X > lo + 1e-9) & (X < hi - 1e-9), axis=1)
        assert interior.any() or X.shape[0] < 30
        assert np.all(w[interior] == 0.0)
        assert np.all(w[~interior] > 0.0)


def test_symbols_exported():
    lib = tl.load_library()
    for name in NEW:
        assert name in tl.exported_symbols()
        assert hasattr(lib, name)


class _NoAbi:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C-ABI")


def _data(E=4, N=20):
    d = tl.GPU_FEAT10_Data(E, N)   # never initialised: no device needed
    d._lib = _NoAbi()
    return d


@pytest.mark.parametrize("make,msg", [
    (lambda: tl.RigidPlane([0, 0, 0], [0, 0, 2], 1e6), "unit length"),
    (lambda: tl.RigidPlane([0, 0, 0], [0, 0, 1 + 1e-9], 1e6), "unit length"),
    (lambda: tl.RigidPlane([0, 0, 0], [0, 0, 1], 0.0), "stiffness must be > 0"),
    (lambda: tl.RigidPlane([0, 0, 0], [0, 0, 1], 1e6, friction=-0.1), "friction must be >= 0"),
    (lambda: tl.RigidPlane([0, 0, 0], [0, 0, 1], 1e6, eps_v=0.0), "eps_v must be > 0"),
    (lambda: tl.RigidPlane([0, 0], [0, 0, 1], 1e6), "point must be a 3-vector"),
    (lambda: tl.RigidPlane([0, 0, np.nan], [0, 0, 1], 1e6), "point must be finite"),
    (lambda: tl.RigidSphere([0, 0, 0], 0.0, 1e6), "radius must be > 0"),
    (lambda: tl.RigidSphere([0, 0, 0], 1.0, -1e6), "stiffness must be > 0"),
])
def test_python_refusals(make, msg):
    with pytest.raises(ValueError, match=msg):
        make()


def test_python_list_refusals():
    p = tl.RigidPlane([0, 0, 0], [0, 0, 1], 1e6)
    with pytest.raises(ValueError, match="at most 16"):
        _data().SetRigidObstacles([p] * 17)
    with pytest.raises(ValueError, match="RigidPlane or RigidSphere"):
        _data().SetRigidObstacles([p, "floor"])
    with pytest.raises(ValueError, match="RigidPlane or RigidSphere"):
        _data().UpdateRigidObstacle(0, None)


def test_obstacle_struct_matches_header():
    names = [f[0] for f in tl.binding.ObstacleC._fields_]
    assert names == ["kind", "p", "n", "radius", "vel", "stiffness", "friction", "eps_v"]
    hdr = open(tl.binding.HEADER_PATH).read()
    assert "tlfea_obstacle;" in hdr


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_rigid_floor_driver_builds(tmp_path):
    lib_dir = os.path.join(ROOT, "total-lagrangian-fea_amd")
    out = tmp_path / "test_sphere_drop_rigid_floor"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(out),
                           os.path.join(HOST, "test_sphere_drop_rigid_floor.cc"), "-L" + lib_dir, "-ltlfea_hip",
                           "-Wl,-rpath," + lib_dir])
    assert out.exists()
