"""The NumPy restatement tests/field_obstacles_np.py of the field obstacles (DESIGN 3e''), pinned without a GPU so that
tests/test_gpu_field_obstacles.py compares the kernels with something already checked: linear reproduction (which ties
it to the pinned plane of tests/obstacles_np.py), the gradient, C1 continuity across cell faces, the convex hull, pose
covariance, the builder against the analytic box distance, and the refusals of the mirror."""
import numpy as np
import pytest

from tests import field_obstacles_np as fnp
from tests import obstacles_np as onp
from tests.helpers import tl

EPS = np.finfo(float).eps
H_STEP = 1e-2
NEW = ("tlfea_set_field_obstacles", "tlfea_update_field_obstacle", "tlfea_clear_field_obstacles",
       "tlfea_get_field_obstacle_resultant", "tlfea_sdf_from_triangles")
SHAPE, ORIGIN, SPACING = (7, 6, 8), np.array([-0.375, -0.25, -0.5]), 0.125  # binary fractions: grid coordinates are exact


def rotation(axis, angle):
    a = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def covered_points(o, n, rng):
    """n world points spread over the coverage of field o"""
    dims = np.array(o["V"].shape[::-1])
    g = 0.5 + rng.random((n, 3)) * (dims - 2.0)
    return (o["rot"] @ (o["origin"] + o["spacing"] * g).T).T + o["pos"]


def smooth_field(rng, **kw):
    return fnp.field(rng.standard_normal(SHAPE[::-1]), ORIGIN, SPACING, 2e6, **kw)


def test_linear_reproduction_ties_to_the_plane():
    rng = np.random.default_rng(1)
    n, p = np.array([0.36, -0.48, 0.8]), np.array([0.02, -0.01, 0.03])
    V = fnp.sample(lambda x: (x - p) @ n, SHAPE, ORIGIN, SPACING)
    o = fnp.field(V, ORIGIN, SPACING, 3e6, mu=0.4, eps_v=0.5, vel=(0.2, 0.1, 0.0))
    plane = dict(kind=0, p=p, n=n, kappa=3e6, mu=0.4, eps_v=0.5, vel=np.array([0.2, 0.1, 0.0]))
    X = covered_points(o, 200, rng)
    vmax = np.abs(V).max()
    F, Fr, B, Br, n_contact = [], [], [], [], 0
    for x in X:
        phi, G = fnp.evaluate(o, x)
        # rounding of the 27-term sums (weights in [0, 1]): 32 EPS of the largest sample, over the spacing for G
        assert abs(phi - n @ (x - p)) <= 32 * EPS * vmax
        assert np.abs(G - n).max() <= 32 * EPS * vmax / SPACING
        x0 = x + 1e-3 * rng.standard_normal(3)
        e0 = fnp.evaluate(o, x0)
        if e0 is None or abs(e0[0]) < 1e-9 or abs(phi) < 1e-9:     # the two gaps could disagree in sign within rounding
            continue
        f, b, act = fnp.force_block(o, 0.01, x, x0, H_STEP)
        fr, br = onp.force_block(plane, 0.01, x, x0, H_STEP)
        n_contact += act
        F, Fr, B, Br = F + [f], Fr + [fr], B + [b], Br + [br]
    F, Fr, B, Br = (np.array(a) for a in (F, Fr, B, Br))
    assert n_contact > 20
    assert np.abs(F - Fr).max() <= 1e-13 * np.abs(Fr).max()
    assert np.abs(B - Br).max() <= 1e-13 * np.abs(Br).max()


def test_gradient_equals_central_differences_within_a_cell():
    rng = np.random.default_rng(2)
    o = smooth_field(rng)
    dims = np.array(SHAPE)
    for _ in range(50):
        i = np.array([rng.integers(1, d - 1) for d in dims])
        t = rng.uniform(-0.3, 0.3, 3)
        x = ORIGIN + SPACING * (i + t)
        phi, G = fnp.evaluate(o, x)
        for a in range(3):
            dx = np.zeros(3)
            dx[a] = 0.15 * SPACING                              # stays inside the cell: phi is quadratic along the axis
            fd = (fnp.evaluate(o, x + dx)[0] - fnp.evaluate(o, x - dx)[0]) / (2 * dx[a])
            assert abs(fd - G[a]) <= 1e-12 * np.abs(o["V"]).max() / SPACING


def test_c1_across_cell_faces():
    rng = np.random.default_rng(3)
    o = smooth_field(rng)
    dims = np.array(SHAPE)
    for _ in range(50):
        a = rng.integers(0, 3)
        i = np.array([rng.integers(1, d - 2) for d in dims])
        g = i + rng.uniform(-0.4, 0.4, 3)
        g[a] = i[a] + 0.5                                       # exactly on the face between samples i and i + 1
        x = ORIGIN + SPACING * g
        hi = i.copy()
        hi[a] += 1
        (p0, G0), (p1, G1) = fnp.evaluate(o, x, force_index=i), fnp.evaluate(o, x, force_index=hi)
        scale = np.abs(o["V"]).max()
        assert abs(p0 - p1) <= 64 * EPS * scale
        assert np.abs(G0 - G1).max() <= 64 * EPS * scale / SPACING


def test_convex_hull():
    rng = np.random.default_rng(4)
    o = fnp.field(rng.uniform(0.1, 2.0, SHAPE[::-1]), ORIGIN, SPACING, 1e6)
    for x in covered_points(o, 200, rng):
        phi, _ = fnp.evaluate(o, x)
        assert 0.1 * (1 - 64 * EPS) <= phi <= 2.0 * (1 + 64 * EPS)
    for t in np.linspace(-0.5, 0.5, 11):
        w, dw = fnp.weights(t)
        assert np.all(w >= 0) and abs(w.sum() - 1) <= 4 * EPS and abs(dw.sum()) <= 4 * EPS


def test_outside_coverage_is_nothing():
    rng = np.random.default_rng(5)
    o = smooth_field(rng, mu=0.3)
    dims = np.array(SHAPE)
    for a in range(3):
        for g_a, inside in ((0.5, True), (0.5 - 1e-12, False), (dims[a] - 1.5, True), (dims[a] - 1.5 + 1e-12, False)):
            g = np.array([2.2, 2.3, 2.4])
            g[a] = g_a
            x = ORIGIN + SPACING * g
            assert (fnp.evaluate(o, x) is not None) == inside
            if not inside:
                f, B, act = fnp.force_block(o, 0.01, x, x, H_STEP)
                assert not f.any() and not B.any() and act == 0


def test_pose_covariance():
    rng = np.random.default_rng(6)
    V = rng.standard_normal(SHAPE[::-1]) - 0.5
    vel = np.array([0.2, -0.1, 0.05])
    R, p = rotation([1, 2, 3], 0.7), np.array([0.4, -0.2, 0.1])
    a = fnp.field(V, ORIGIN, SPACING, 2e6, mu=0.4, eps_v=0.5, vel=vel)
    b = fnp.field(V, ORIGIN, SPACING, 2e6, mu=0.4, eps_v=0.5, vel=R @ vel, pos=p, rot=R)
    X = covered_points(a, 100, rng)
    hits = 0
    for x in X:
        x0 = x + 1e-3 * rng.standard_normal(3)
        fa, Ba, acta = fnp.force_block(a, 0.02, x, x0, H_STEP)
        fb, Bb, actb = fnp.force_block(b, 0.02, R @ x + p, R @ x0 + p, H_STEP)
        hits += acta
        assert acta == actb
        assert np.abs(R @ fa - fb).max() <= 1e-12 * max(np.abs(fa).max(), 1e-300)
        assert np.abs(R @ Ba @ R.T - Bb).max() <= 1e-12 * max(np.abs(Ba).max(), 1e-300)
    assert hits > 10


def test_force_is_the_gradient_of_the_energy():
    rng = np.random.default_rng(7)
    o = smooth_field(rng)
    n = 0
    for x in covered_points(o, 60, rng):
        phi, G = fnp.evaluate(o, x)
        if phi > -0.05:
            continue
        n += 1
        f, _, _ = fnp.force_block(o, 0.02, x, x, H_STEP)
        for a in range(3):
            dx = np.zeros(3)
            dx[a] = 1e-6
            fd = -(fnp.energy(o, 0.02, x + dx) - fnp.energy(o, 0.02, x - dx)) / 2e-6
            assert abs(fd - f[a]) <= 1e-5 * np.abs(f).max() + 1e-6
    assert n > 5


LO, HI = np.array([-0.2, -0.15, -0.1]), np.array([0.25, 0.2, 0.15])


@pytest.mark.parametrize("sub", (1, 2))
def test_builder_against_the_box_distance(sub):
    V, T = fnp.box_triangles(LO, HI, sub)
    assert len(T) == 12 * sub * sub and fnp.check_closed(V, T) == ""
    shape, origin, spacing = (6, 5, 5), LO - 0.137, 0.149    # no sample lies on the surface
    S = fnp.sdf_grid(V, T, shape, origin, spacing)
    ref = fnp.box_distance(fnp.sample(lambda x: x, shape, origin, spacing), LO, HI)
    assert np.abs(ref).min() > 1e-3 and (ref < 0).any() and (ref > 0).any()
    assert np.array_equal(np.sign(S), np.sign(ref))
    assert np.abs(S - ref).max() <= 1e-13 * np.linalg.norm(HI - LO)


def test_winding_numbers_are_integers():
    rng = np.random.default_rng(8)
    V, T = fnp.box_triangles(LO, HI, 2)
    for Tk in (T, T[:, ::-1]):                                   # either orientation
        for p in rng.uniform(LO - 0.3, HI + 0.3, (40, 3)):
            d, wn = fnp.sdf_point(p, V, Tk)
            inside = fnp.box_distance(p, LO, HI) < 0
            assert abs(abs(wn) - (1.0 if inside else 0.0)) <= 1e-12
            assert (d < 0) == inside


def test_mirror_refuses_open_and_flipped_surfaces():
    from importlib import import_module
    obs = import_module(tl.__name__ + ".obstacles")
    V, T = fnp.box_triangles(LO, HI, 1)
    obs.check_closed_surface(V, T)
    with pytest.raises(ValueError, match="open"):
        obs.check_closed_surface(V, T[:-1])
    flipped = T.copy()
    flipped[3] = flipped[3, ::-1]
    with pytest.raises(ValueError, match="consistently oriented"):
        obs.check_closed_surface(V, flipped)
    degenerate = T.copy()
    degenerate[0] = [T[0, 0], T[0, 0], T[0, 1]]
    with pytest.raises(ValueError):
        obs.check_closed_surface(V, degenerate)
    bad = T.copy()
    bad[0, 0] = len(V)
    with pytest.raises(ValueError, match="indices"):
        obs.check_closed_surface(V, bad)
    assert fnp.check_closed(V, T[:-1]) == "open surface" and fnp.check_closed(V, flipped) == "inconsistent orientation"


def test_mirror_checks_the_field():
    good = fnp.sample(lambda x: np.linalg.norm(x, axis=-1) - 0.1, SHAPE, ORIGIN, SPACING)
    assert fnp.closed_shape_ok(good)
    f = tl.RigidField(good, ORIGIN, SPACING, 1e6)
    assert f.shape == SHAPE and f.to_c().nx == 7 and f.to_c().nz == 8
    with pytest.raises(ValueError, match="5 samples"):
        tl.RigidField(good[:, :4], ORIGIN, SPACING, 1e6)
    bad = good.copy()
    bad[3, 3, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        tl.RigidField(bad, ORIGIN, SPACING, 1e6)
    for idx in ((1, 3, 3), (3, 4, 3), (3, 3, 5), (0, 0, 0)):
        bad = good.copy()
        bad[idx] = -0.01
        assert not fnp.closed_shape_ok(bad)
        with pytest.raises(ValueError, match="outermost"):
            tl.RigidField(bad, ORIGIN, SPACING, 1e6)
    for kw in (dict(spacing=0.0), dict(stiffness=0.0), dict(friction=-1.0), dict(eps_v=0.0),
               dict(rotation=np.eye(3) * 1.001), dict(rotation=np.diag([1.0, 1.0, -1.0])), dict(position=[0, np.inf, 0])):
        args = dict(values=good, origin=ORIGIN, spacing=SPACING, stiffness=1e6)
        args.update(kw)
        with pytest.raises(ValueError):
            tl.RigidField(**args)
    with pytest.raises(ValueError, match="margin"):
        tl.RigidField.from_triangles(*fnp.box_triangles(LO, HI, 1), 0.05, 1e6, margin=2.0)
    g = tl.RigidField.from_function(lambda x: np.linalg.norm(x, axis=-1) - 0.1, [-0.4] * 3, [0.4] * 3, 0.1, 1e6)
    assert g.shape == (9, 9, 9)
    m = f.moved(position=[0.0, 0.0, 0.1])
    assert m.values is f.values and m.position[2] == 0.1 and f.position[2] == 0.0


def test_symbols_and_members():
    import ctypes as C
    syms = tl.exported_symbols()
    assert all(s in syms for s in NEW)
    assert C.sizeof(tl.binding.FieldObstacleC) == 192
    for cls in (tl.GPU_FEAT10_Data, tl.GPU_ANCF3243_Data, tl.GPU_ANCF3443_Data):
        for name in ("SetFieldObstacles", "UpdateFieldObstacle", "ClearFieldObstacles", "GetFieldObstacleResultant"):
            assert hasattr(cls, name), name
    assert hasattr(tl.GPU_FEAT10_Data, "GetBoundaryTriangles")
    with pytest.raises(ValueError, match="RigidPlane or RigidSphere"):
        import importlib
        importlib.import_module(tl.__name__ + ".obstacles").as_c(
            tl.RigidField(fnp.sample(lambda x: np.linalg.norm(x, axis=-1) - 0.1, SHAPE, ORIGIN, SPACING), ORIGIN, SPACING, 1e6))
