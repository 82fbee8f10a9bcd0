"""Field obstacles on the GPU (DESIGN 3e''): kernel parity with tests/field_obstacles_np.py (pinned without a GPU by
tests/test_field_obstacles_np.py) on T10 and ANCF meshes, alone and beside analytic obstacles, with points placed by hand
where the kernel can go wrong; the Hessian; resting equilibrium on the flat top of a field box; the solvers; a moving
pose; bitwise checks; the refusals; and the builder on the device.  Tolerances are those of tests/test_gpu_obstacles.py
and tests/test_gpu_ancf_obstacles.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import ancf_obstacles_np as aonp
from tests import field_obstacles_np as fnp
from tests import obstacles_np as onp
from tests.helpers import MESHES, csr_to_dense, load_mesh, make_gpu, tl
from tests.test_gpu_ancf_obstacles import coefs, gravity_load, move
from tests.test_gpu_ancf_stress import SHAPES, make_ancf_gpu
from tests.test_gpu_obstacles import G, SOFT, as_dict, body, newton, plane, positions

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
H_STEP = 1e-2


def rotation(axis, angle):
    a = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def sphere_field(shape, spacing, radius, kappa, **kw):
    """A sphere of `radius` about the frame's origin sampled on a grid of `shape` samples centred on it.  On the
    anisotropic 7 x 6 x 8 grid the closed-shape rule needs radius < 1.5 spacings (the y axis has two inner samples)."""
    origin = -0.5 * (np.array(shape) - 1.0) * spacing
    V = fnp.sample(lambda x: np.linalg.norm(x, axis=-1) - radius, shape, origin, spacing)
    return tl.RigidField(V, origin, spacing, kappa, **kw)


def to_dict(o):
    if isinstance(o, tl.RigidField):
        return fnp.field(o.values, o.origin, o.spacing, o.stiffness, mu=o.friction, eps_v=o.eps_v, pos=o.position,
                         rot=o.rotation, vel=o.velocity)
    return as_dict(o)


def box_field(lo, hi, spacing, kappa, margin=3, **kw):
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    return tl.RigidField.from_function(lambda p: fnp.box_distance(p, lo, hi), lo - margin * spacing, hi + margin * spacing,
                                       spacing, kappa, **kw)


# ---- 1. kernel parity -------------------------------------------------------------------------------------------------
def t10_scene():
    """res2 (a 3 x 2 x 1 block, surface nodes every 0.25).  Field A: the 7 x 6 x 8 sphere, rotated, with friction and a
    velocity, dipping into the top face.  Field B: identity pose on a grid of binary fractions under the bottom face, so
    that grid coordinates are exact: the bottom nodes near it sit exactly at samples in x and y (t = 0) and on a cell face
    in z (t = 1/2); single nodes are moved onto the coverage boundary (g = 0.5, g = n - 1.5), just outside it, and to a
    generic place inside the body; one node inside the body is pinned."""
    X, conn = load_mesh("res2")
    rng = np.random.default_rng(3)
    A = sphere_field((7, 6, 8), 0.5, 0.7, 3e7, friction=0.4, eps_v=0.5, velocity=[0.2, 0.1, 0.0],
                     position=[1.5, 1.0, 1.45], rotation=rotation([1, 2, 3], 0.4))
    shape_b, sp_b, org_b = (7, 6, 6), 0.25, np.array([1.5, 0.25, -0.625])
    c_b = org_b + sp_b * np.array([3.0, 2.5, 2.5])                      # (2.25, 0.875, 0): on the bottom face
    Vb = fnp.sample(lambda x: np.linalg.norm(x - c_b, axis=-1) - 0.35, shape_b, org_b, sp_b)
    B = tl.RigidField(Vb, org_b, sp_b, 5e7, friction=0.3, eps_v=0.5, velocity=[0.0, -0.1, 0.05])
    xp = X + rng.normal(0, 2e-2, X.shape)
    x = xp + rng.normal(0, 5e-3, X.shape)
    near = np.nonzero((np.abs(X[:, 2]) < 1e-12) & (X[:, 0] >= 1.5) & (X[:, 1] >= 0.25) & (X[:, 1] <= 1.5))[0]
    x[near] = xp[near] = X[near]

    def node(px, py):
        i = np.nonzero((np.abs(X[:, 0] - px) < 1e-12) & (np.abs(X[:, 1] - py) < 1e-12) & (np.abs(X[:, 2]) < 1e-12))[0]
        assert i.size == 1
        return int(i[0])

    x[node(1.75, 0.75), 0] = xp[node(1.75, 0.75), 0] = 1.625            # g_x = 0.5: on the coverage boundary
    x[node(3.0, 0.75), 0] = xp[node(3.0, 0.75), 0] = 2.875              # g_x = n_x - 1.5
    x[node(1.75, 1.0), 0] = xp[node(1.75, 1.0), 0] = 1.625 - 2.0 ** -30  # just outside
    x[node(2.25, 1.0)] += np.array([0.01, -0.004, -0.03])               # generic t, deeper, sliding
    x[node(2.5, 0.75), 2] = -0.02                                       # t_x = t_y = 0 exactly, generic t_z
    pinned = np.array([node(2.25, 0.75)], dtype=np.int32)               # 0.125 from the centre: inside the body
    special = dict(lo=node(1.75, 0.75), hi=node(3.0, 0.75), out=node(1.75, 1.0), face=node(2.0, 0.75))
    return X, conn, [A, B], xp, x, pinned, special


def t10_eval(X, conn, xp, x, pinned, analytic, fields):
    d = make_gpu(X, conn, SOFT, fixed=pinned)
    if analytic:
        d.SetRigidObstacles(analytic)
    if fields:
        d.SetFieldObstacles(fields)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-7, 0.0, 1e-6, 1e14, 1, 40, H_STEP))
    s.SetLinSolveOpts(tl.LinSolveOpts(rel_tol=1e-13, max_iter=50000))
    s.AnalyzeHessianSparsity()
    d.UpdatePositions(xp[:, 0], xp[:, 1], xp[:, 2])
    s.BeginStep()
    d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])
    s.EvalGradient()
    out = dict(g=s.RetrieveGradientToCPU())
    s.AssembleHessian()
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    out.update(H=csr_to_dense(ro, ci, val, 3 * X.shape[0]), val=val, f=d.GetObstacleForces(), w=d.GetSurfaceWeights(),
               res_a=[d.GetObstacleResultant(k) for k in range(len(analytic))],
               res_f=[d.GetFieldObstacleResultant(k) for k in range(len(fields))])
    del s
    d.Destroy()
    return out


def test_t10_kernel_parity_and_hessian():
    X, conn, fields, xp, x, pinned, special = t10_scene()
    N = X.shape[0]
    analytic = [plane([0, 0, 0.05], [0.01, 0.005, 1.0], 3e7, friction=0.4, eps_v=0.5, velocity=[0.2, 0.1, 0.0]),
                tl.RigidSphere([3.1, 2.1, 1.1], 0.35, 5e7, friction=0.3, eps_v=0.5, velocity=[0.0, -0.1, 0.05])]
    none = t10_eval(X, conn, xp, x, pinned, [], [])
    w = onp.surface_weights(X, conn)
    # the places chosen by hand are what they are meant to be
    B = to_dict(fields[1])
    assert fnp.grid_coords(B, x[special["lo"]])[0] == 0.5 and fnp.grid_coords(B, x[special["hi"]])[0] == 7 - 1.5
    assert fnp.evaluate(B, x[special["lo"]]) is not None and fnp.evaluate(B, x[special["hi"]]) is not None
    # ... where the spline is evaluated (index clamped to n - 2 at the upper end) and positive by the closed-shape rule
    assert 0 < fnp.evaluate(B, x[special["lo"]])[0] < np.inf and 0 < fnp.evaluate(B, x[special["hi"]])[0] < np.inf
    assert fnp.evaluate(B, x[special["out"]]) is None
    gf = fnp.grid_coords(B, x[special["face"]])
    assert gf[0] == 2.0 and gf[1] == 2.0 and gf[2] == 2.5 and fnp.evaluate(B, x[special["face"]])[0] < 0
    assert fnp.evaluate(B, x[pinned[0]])[0] < 0
    for ana in ([], analytic):
        got = t10_eval(X, conn, xp, x, pinned, ana, fields)
        assert np.allclose(got["w"], w, rtol=1e-13, atol=0)
        obs = [to_dict(o) for o in ana + fields]
        F, Bk, res = fnp.nodal(obs, w, x, xp, H_STEP, pinned=pinned)
        Ff, _, _ = fnp.nodal(obs[len(ana):], w, x, xp, H_STEP, pinned=pinned)
        assert np.count_nonzero(np.linalg.norm(Ff, axis=1)) >= 12
        assert not F[pinned].any() and not Ff[special["out"]].any() and not Ff[special["lo"]].any() and not Ff[special["hi"]].any()
        fscale = np.abs(F).max()
        err = {"force": np.max(np.abs(got["f"] - F.reshape(-1))) / fscale,
               "g": np.max(np.abs((got["g"] - none["g"]) + F.reshape(-1))) / max(fscale, np.abs(none["g"]).max())}
        print("t10", len(ana), {k: f"{v:.2e}" for k, v in err.items()})
        assert err["force"] <= 1e-13 and err["g"] <= 1e-13
        assert not got["f"].reshape(-1, 3)[pinned].any()
        if not ana:                                  # outside coverage, and on its boundary where phi > 0: exactly nothing
            assert not got["f"].reshape(-1, 3)[[special["out"], special["lo"], special["hi"]]].any()
        for k, (r, n_act) in enumerate(got["res_a"] + got["res_f"]):
            assert np.max(np.abs(r - res[k][0])) <= 1e-13 * fscale, k
            assert n_act == res[k][1], k
        assert sum(c for _, c in res[len(ana):]) >= 12
        # Hessian: h B on the diagonal blocks of surface nodes, nothing elsewhere
        dH = got["H"] - none["H"]
        bscale = H_STEP * np.abs(Bk).max()
        for i in range(N):
            assert np.max(np.abs(dH[3 * i:3 * i + 3, 3 * i:3 * i + 3] - H_STEP * Bk[i])) <= 1e-13 * bscale
            dH[3 * i:3 * i + 3, 3 * i:3 * i + 3] = 0.0
        assert np.max(np.abs(dH)) <= 1e-13 * np.abs(none["H"]).max()
        if not ana:                                  # rows of nodes without a block: the bits of the run without obstacles
            quiet = [i for i in range(N) if not Bk[i].any()]
            assert 0 < len(quiet) < N
            rows = np.concatenate([np.arange(3 * i, 3 * i + 3) for i in quiet])
            assert np.array_equal(got["H"][rows], none["H"][rows])


def ancf_scene(shape):
    """The shape's reference state perturbed as in tests/test_gpu_ancf_obstacles.scene; a 7 x 6 x 8 sphere field, rotated,
    with friction and a velocity, dipping into the upper face above the node nearest to the centroid; beside it for the mixed run a half-space under part of the mesh and an analytic sphere."""
    prob = SHAPES[shape]()
    beam = prob[0] == 3243
    X = aonp.reference(prob)
    nodes = X[0::4]
    # The friction terms divide by the slip |u| or by eps_v h, which are differences of coordinates.  On the net (10 m)
    # one ulp of the coordinates against a slip of 5e-3 moves the restated Hessian itself by 1.2e-12 of its largest
    # entry (measured: both states perturbed by a random ulp), twelve times the 1e-13 bound; the shapes up to 4 m
    # stay at 1.1e-13 (beam5) and below.  So on a mesh beyond 5 m slip, obstacle velocities and eps_v are 20 times
    # larger, which brings the net's figure to 6.3e-14.
    k = 20.0 if np.abs(X).max() > 5.0 else 1.0
    c = nodes[np.argmin(np.linalg.norm(nodes - nodes.mean(axis=0), axis=1))]
    # on so coarse a grid the interpolant's zero set lies about spacing^2 / (4 R) inside the sphere: the field dips deeper
    R, dip, fdip = (0.2, 0.03, 0.08) if beam else (2.0, 0.08, 0.5)
    up = np.array([0.0, 0.0, 0.5 * prob[5][2] + R - dip])
    fld = sphere_field((7, 6, 8), R / 1.4, R, 5e7, friction=0.3, eps_v=0.5 * k, velocity=[0.0, -0.1 * k, 0.05 * k],
                       position=c + up - [0.0, 0.0, fdip - dip], rotation=rotation([2, -1, 3], 0.5))
    lo = nodes[np.argmin(nodes[:, 0])]
    analytic = [plane([lo[0] + 0.4 * (nodes[:, 0].max() - lo[0]), lo[1], lo[2]], [0.2 if beam else 0.1, 0.0, 1.0], 3e7,
                      friction=0.4, eps_v=0.5 * k, velocity=[0.2 * k, 0.1 * k, 0.0]),
                tl.RigidSphere(nodes[np.argmax(nodes[:, 0])] + up, R, 5e7)]
    rng = np.random.default_rng(11)
    xp = X + rng.normal(0, 2e-3, X.shape)
    x = xp + rng.normal(0, 1e-4, X.shape)
    x[0::4] += k * np.array([0.004, -0.003, 0.0])
    return prob, fld, analytic, xp, x


@functools.lru_cache(maxsize=None)
def ancf_reference(shape, mixed):
    prob, fld, analytic, xp, x = ancf_scene(shape)
    return fnp.ancf_assemble(prob, [to_dict(o) for o in (analytic if mixed else []) + [fld]], x, xp, H_STEP)


def ancf_eval(prob, xp, x, analytic, fields):
    d = make_ancf_gpu(prob, SOFT)
    if analytic:
        d.SetRigidObstacles(analytic)
    if fields:
        d.SetFieldObstacles(fields)
    s = newton(d, H_STEP)
    s.AnalyzeHessianSparsity()
    move(d, xp)
    s.BeginStep()
    move(d, x)
    s.EvalGradient()
    out = dict(g=s.RetrieveGradientToCPU())
    s.AssembleHessian()
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    out.update(ro=ro, ci=ci, val=val)
    if analytic or fields:
        out.update(f=d.GetObstacleForces(), pts=d.RetrieveContactPointsToCPU(),
                   res=[d.GetObstacleResultant(k) for k in range(len(analytic))] +
                       [d.GetFieldObstacleResultant(k) for k in range(len(fields))])
    del s
    d.Destroy()
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_ancf_kernel_parity_and_tangent(shape):
    prob, fld, analytic, xp, x = ancf_scene(shape)
    none = ancf_eval(prob, xp, x, [], [])
    for mixed in (False, True):
        ref = ancf_reference(shape, mixed)
        got = ancf_eval(prob, xp, x, analytic if mixed else [], [fld])
        dH = fnp.coo_on_csr(none["ro"], none["ci"], ref["hessian_coo"], 3 * x.shape[0])
        assert ref["resultants"][-1][1] >= 4                       # the field touches sample points
        F = ref["force"].reshape(-1)
        fscale = np.abs(F).max()
        cov = np.isfinite(ref["gap"])
        assert np.array_equal(np.isfinite(got["pts"][:, :, 3]), cov)
        assert cov.any() and (mixed or prob[0] != 3243 or not cov.all())   # a beam line has points the field does not cover
        err = {"force": np.max(np.abs(got["f"] - F)) / fscale,
               "g": np.max(np.abs((got["g"] - none["g"]) + F)) / max(fscale, np.abs(none["g"]).max()),
               "H": np.max(np.abs((got["val"] - none["val"]) - dH)) / max(np.abs(dH).max(), np.abs(none["val"]).max()),
               "points": np.max(np.abs(got["pts"][:, :, :3] - ref["points"])) / np.abs(ref["points"]).max(),
               "gap": np.max(np.abs(got["pts"][:, :, 3][cov] - ref["gap"][cov])) / np.abs(ref["gap"][cov]).max(),
               "pressure": np.max(np.abs(got["pts"][:, :, 4] - ref["pressure"])) / ref["pressure"].max()}
        print(shape, mixed, {k: f"{v:.2e}" for k, v in err.items()})
        for name, v in err.items():
            assert v <= 1e-13, name
        assert np.all(np.isposinf(got["pts"][:, :, 3][~cov]))
        # the resultants' own largest row: a sum over up to 10816 points (the net's plane) is larger than any single force
        rscale = max(fscale, max(np.abs(rk).max() for rk, _ in ref["resultants"]))
        for k, (r, n_act) in enumerate(got["res"]):
            print(shape, mixed, "resultant", k, np.max(np.abs(r - ref["resultants"][k][0])) / rscale)
            assert np.max(np.abs(r - ref["resultants"][k][0])) <= 1e-13 * rscale, k
            assert n_act == ref["resultants"][k][1], k
        # rows of coefficients all of whose elements are untouched: the bits of the run without obstacles
        ids = aonp.coef_ids(prob)
        free = np.setdiff1d(np.arange(x.shape[0]), ids[ref["touched"]].reshape(-1))
        ro = none["ro"]
        for i in free:
            assert np.array_equal(none["val"][ro[3 * i]:ro[3 * i + 3]], got["val"][ro[3 * i]:ro[3 * i + 3]]), i
        if not mixed and prob[4].shape[0] >= 5:
            assert free.size > 0


# ---- 3. resting equilibrium ---------------------------------------------------------------------------------------------
def floor_box(top, kappa, **kw):
    """A box far wider than the meshes (they span [0, 3.2] x [0, 2]) with its top face at z = top.  Spacing 0.5: the samples
    around the top face under the meshes are z - top exactly, so the interpolant is exact there."""
    return box_field([-2.5, -2.5, top - 1.5], [5.5, 4.5, top], 0.5, kappa, **kw)


def t10_rest(fields, h=0.05, steps=40, gravity=(0.0, 0.0, -G), method=0):
    X, conn = load_mesh("beam_3x2x1")
    d, mass = body(X, conn, gravity)
    d.SetFieldObstacles(fields)
    s = newton(d, h, method=method)
    for _ in range(steps):
        s.Solve()
    return d, s, mass


def ancf_rest(fields, gvec=(0.0, 0.0, -G), h=0.05, steps=40, method=0):
    d = make_ancf_gpu(SHAPES["plate2x2"](), SOFT)
    f, mass = gravity_load(d, gvec)
    d.SetExternalForce(f)
    d.SetFieldObstacles(fields)
    s = newton(d, h, method=method)
    for _ in range(steps):
        s.Solve()
    return d, s, mass


def test_resting_box_weight_on_a_field():
    kappa = 1e8
    fld = floor_box(0.0, kappa)
    o = to_dict(fld)
    for p in ([0.3, 0.2, -1e-4], [2.9, 1.7, 2e-4], [1.5, 1.0, 0.2]):      # linear in z under the beam
        phi, Gr = fnp.evaluate(o, np.array(p))
        assert abs(phi - p[2]) <= 8 * EPS and np.max(np.abs(Gr - [0, 0, 1])) <= 32 * EPS
    d, s, mass = t10_rest([fld])
    W = mass.sum() * G
    r, n_act = d.GetFieldObstacleResultant(0)
    print("t10 rest", r, n_act, W, s.GetStats() if hasattr(s, "GetStats") else "")
    assert n_act > 0
    assert abs(r[2] - W) <= 1e-8 * W
    assert np.max(np.abs(r[:2])) <= 1e-8 * W
    x = positions(d)
    pen = np.sum(d.GetSurfaceWeights() * np.maximum(-x[:, 2], 0.0))
    assert abs(pen - W / kappa) <= 1e-8 * W / kappa
    del s
    d.Destroy()


def test_resting_plate_weight_on_a_field():
    d, s, mass = ancf_rest([floor_box(-0.05, 1e8)])
    Wt = mass * G
    r, n_act = d.GetFieldObstacleResultant(0)
    print("plate rest", r, n_act, Wt)
    assert n_act > 0
    assert abs(r[2] - Wt) <= 1e-8 * Wt
    assert np.max(np.abs(r[:2])) <= 1e-8 * Wt
    pts, w = d.RetrieveContactPointsToCPU(), d.GetSurfacePointWeights()
    pen = np.sum(w * np.maximum(-pts[:, :, 3], 0.0))
    assert abs(pen - Wt / 1e8) <= 1e-8 * Wt / 1e8
    del s
    d.Destroy()


# ---- 4. solvers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["t10", "ancf"])
def test_direct_equals_iterative(kind):
    xs = []
    for method in (0, 1):
        if kind == "t10":
            d, s, _ = t10_rest([floor_box(0.0, 1e8, friction=0.3, eps_v=1e-2)], steps=10, gravity=(2.0, 0.0, -G), method=method)
            xs.append(positions(d))
        else:
            d, s, _ = ancf_rest([floor_box(-0.05, 1e8, friction=0.3, eps_v=1e-2)], gvec=(2.0, 0.0, -G), steps=10, method=method)
            xs.append(coefs(d))
        del s
        d.Destroy()
    assert np.max(np.abs(xs[0] - xs[1])) <= 1e-10 * np.max(np.abs(xs[0]))


@pytest.mark.parametrize("solver", ["adamw", "nesterov"])
def test_first_order_solvers_hold_the_weight(solver):
    X, conn = load_mesh("beam_3x2x1")
    fld = floor_box(0.0, 1e8)
    d0, s0, mass = t10_rest([fld])
    xr = positions(d0)
    del s0
    d0.Destroy()
    W = mass.sum() * G
    d, _ = body(X, conn)
    d.SetFieldObstacles([fld])
    d.UpdatePositions(xr[:, 0], xr[:, 1], xr[:, 2])
    if solver == "adamw":
        s = tl.SyncedAdamWNocoopSolver(d, 0)
        s.SetParameters(tl.SyncedAdamWNocoopParams(max_outer=1, max_inner=50, time_step=1e-3))
    else:
        s = tl.SyncedNesterovSolver(d, 0)
        s.SetParameters(tl.SyncedNesterovParams(max_outer=1, max_inner=20, time_step=1e-3))
    s.Setup()
    s.Solve()
    r, _ = d.GetFieldObstacleResultant(0)
    print(solver, r, W)
    assert abs(r[2] - W) <= 1e-4 * W
    assert np.max(np.abs(positions(d) - xr)) <= 1e-6
    del s
    d.Destroy()


# ---- 5. moving pose ---------------------------------------------------------------------------------------------------------
def test_update_equals_a_field_with_the_shifted_origin():
    X, conn = load_mesh("beam_3x2x1")
    dz = 0.0078125                                                     # 2^-7: the shifted origin is exact
    fld = floor_box(0.0, 1e8, friction=0.3, eps_v=1e-2)
    shifted = tl.RigidField(fld.values, fld.origin + [0, 0, dz], fld.spacing, 1e8, friction=0.3, eps_v=1e-2)
    xs = []
    for update in (True, False):
        d, mass = body(X, conn, (1.0, 0.0, -G))
        d.SetFieldObstacles([fld])
        s = newton(d, 0.05)
        for _ in range(3):
            s.Solve()
        x_before = positions(d)
        if update:
            d.UpdateFieldObstacle(0, fld.moved(position=[0, 0, dz]))
        else:
            d.SetFieldObstacles([shifted])
        for _ in range(3):
            s.Solve()
        xs.append(positions(d))
        r, n_act = d.GetFieldObstacleResultant(0)
        assert n_act > 0 and r[2] > 0
        del s
        d.Destroy()
    disp = np.max(np.abs(xs[0] - x_before))
    err = np.max(np.abs(xs[0] - xs[1]))
    print("moving pose", err, disp)
    assert disp > 0.5 * dz
    assert err <= 1e-10 * disp + 8 * EPS * np.max(np.abs(xs[0]))


# ---- 6. determinism and the untouched path --------------------------------------------------------------------------------
def test_determinism():
    X, conn, fields, xp, x, pinned, _ = t10_scene()
    runs = []
    for _ in range(2):
        got = t10_eval(X, conn, xp, x, pinned, [], fields)
        runs.append((got["g"], got["val"], got["f"], got["res_f"][0][0], got["res_f"][1][0]))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", ["beam5", "plate2x2"])
def test_ancf_determinism(shape):
    """points, gather, tangent and footprint kernels with a field and analytic obstacles: two runs, the same bits"""
    prob, fld, analytic, xp, x = ancf_scene(shape)
    runs = []
    for _ in range(2):
        got = ancf_eval(prob, xp, x, analytic, [fld])
        runs.append([got["g"], got["val"], got["f"], got["pts"]] + [r for r, _ in got["res"]])
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


def test_set_then_clear_is_bitwise_untouched_and_lists_are_independent():
    X, conn = load_mesh("beam_3x2x1")
    fld = floor_box(0.5, 1e8)
    floor = plane([0, 0, 0.01], [0, 0, 1], 1e8)
    xs = []
    for touch in ("never", "field", "plane only", "plane after both"):
        d, _ = body(X, conn)
        if touch == "field":
            d.SetFieldObstacles([fld])
            d.ClearFieldObstacles()
        elif touch == "plane only":
            d.SetRigidObstacles([floor])
        elif touch == "plane after both":                            # clearing one list keeps the other
            d.SetFieldObstacles([fld])
            d.SetRigidObstacles([floor])
            d.ClearFieldObstacles()
        s = newton(d, 1e-2)
        s.Solve()
        s.AssembleHessian()
        xs.append((positions(d), s.RetrieveGradientToCPU(), s.RetrieveHessianCSRToCPU()[2]))
        if touch == "plane after both":
            assert d.GetObstacleResultant(0)[1] > 0
            with pytest.raises(tl.TlfeaError, match="outside the 0 field"):
                d.GetFieldObstacleResultant(0)
            d.SetFieldObstacles([fld])
            d.ClearRigidObstacles()                                  # ... and the other way round
            s.Solve()
            assert d.GetFieldObstacleResultant(0)[1] > 0
            with pytest.raises(tl.TlfeaError, match="outside the 0 obstacles"):
                d.GetObstacleResultant(0)
        del s
        d.Destroy()
    for a, b in ((0, 1), (2, 3)):
        for u, v in zip(xs[a], xs[b]):
            assert np.array_equal(u, v)
    assert not np.array_equal(xs[0][0], xs[2][0])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_object_usable():
    lib = tl.load_library()
    X, conn = load_mesh("beam_3x2x1")
    d, mass = body(X, conn)
    good = floor_box(0.0, 1e8)
    one, ptr = good.to_c(), (tl.binding.c_dp * 1)(tl.binding.dp(good.values))

    def refused(o, values, n, msg):
        assert lib.tlfea_set_field_obstacles(d._h, C.byref(o) if o is not None else None, values, n) != 0
        assert msg in lib.tlfea_last_error().decode(), lib.tlfea_last_error().decode()

    many = (tl.binding.FieldObstacleC * 17)(*[one] * 17)
    ptrs = (tl.binding.c_dp * 17)(*[tl.binding.dp(good.values)] * 17)
    assert lib.tlfea_set_field_obstacles(d._h, many, ptrs, 17) != 0 and "0..16" in lib.tlfea_last_error().decode()
    assert lib.tlfea_set_field_obstacles(d._h, many, ptrs, -1) != 0 and "0..16" in lib.tlfea_last_error().decode()
    refused(None, ptr, 1, "null list")
    refused(one, None, 1, "null sample pointer")
    refused(one, (tl.binding.c_dp * 1)(None), 1, "null sample pointer")
    for field, value, msg in (("nx", 4, "at least 5"), ("spacing", 0.0, "spacing"), ("stiffness", 0.0, "stiffness"),
                              ("friction", -1.0, "friction"), ("eps_v", 0.0, "eps_v"), ("nz", 1 << 20, "2^27")):
        o = good.to_c()
        setattr(o, field, value)
        refused(o, ptr, 1, msg)
    o = good.to_c()
    o.rot[0] = 1.0 + 1e-9
    refused(o, ptr, 1, "orthonormal")
    o = good.to_c()
    o.rot[0] = -1.0
    refused(o, ptr, 1, "determinant")
    for idx, value, msg in (((3, 3, 3), np.inf, "non-finite sample"), ((1, 4, 4), -0.1, "outermost"),
                            ((4, 4, good.values.shape[2] - 2), 0.0, "outermost")):
        bad = good.values.copy()
        bad[idx] = value
        refused(one, (tl.binding.c_dp * 1)(tl.binding.dp(bad)), 1, msg)
    # more than 16 together with the analytic list: whichever call comes second
    floor = plane([0, 0, -1.0], [0, 0, 1], 1e8)
    d.SetRigidObstacles([floor] * 10)
    assert lib.tlfea_set_field_obstacles(d._h, many, ptrs, 7) != 0 and "exceed" in lib.tlfea_last_error().decode()
    d.SetFieldObstacles([good] * 6)
    with pytest.raises(tl.TlfeaError, match="exceed"):
        d.SetRigidObstacles([floor] * 11)
    d.ClearRigidObstacles()
    d.SetFieldObstacles([good])
    with pytest.raises(tl.TlfeaError, match="outside the 1 field"):
        d.UpdateFieldObstacle(1, good)
    with pytest.raises(tl.TlfeaError, match="outside the 1 field"):
        d.GetFieldObstacleResultant(-1)
    other = box_field([-2.5, -2.5, -1.5], [5.5, 4.5, 0.0], 0.25, 1e8)
    with pytest.raises(tl.TlfeaError, match="stored one"):
        d.UpdateFieldObstacle(0, other)
    with pytest.raises(ValueError, match="RigidPlane or RigidSphere"):
        d.SetRigidObstacles([good])
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
    # before Setup, and for ANCF before CalcDsDuPre
    raw = tl.GPU_FEAT10_Data(conn.shape[0], X.shape[0])
    raw.Initialize()
    with pytest.raises(tl.TlfeaError, match="set up"):
        raw.SetFieldObstacles([good])
    raw.Destroy()
    kind, xa, ya, za, conn_a, (L, W, H) = SHAPES["plate2x2"]()
    q = tl.quadrature
    a = tl.GPU_ANCF3443_Data(len(xa) // 4, conn_a.shape[0])
    a.Initialize()
    a.Setup(L, W, H, q.gauss_xi_m_7, q.gauss_eta_m_7, q.gauss_zeta_m_3, q.gauss_xi_4, q.gauss_eta_4, q.gauss_zeta_3,
            q.weight_xi_m_7, q.weight_eta_m_7, q.weight_zeta_m_3, q.weight_xi_4, q.weight_eta_4, q.weight_zeta_3, xa, ya, za,
            conn_a)
    with pytest.raises(tl.TlfeaError, match="CalcDsDuPre"):
        a.SetFieldObstacles([good])
    a.Destroy()
    # the builder
    V, T = fnp.box_triangles([0, 0, 0], [1, 1, 1], 1)
    out = np.zeros(125)

    def build(Vk, Tk):
        Vk, Tk = np.ascontiguousarray(Vk, dtype=np.float64), np.ascontiguousarray(Tk, dtype=np.int32)
        org = np.array([-0.5, -0.5, -0.5])
        return lib.tlfea_sdf_from_triangles(tl.binding.dp(Vk), len(Vk), tl.binding.ip(Tk), len(Tk), 5, 5, 5,
                                            tl.binding.dp(org), C.c_double(0.5), tl.binding.dp(out))

    assert build(V, T) == 0
    flipped, degenerate, outside = T.copy(), T.copy(), T.copy()
    flipped[3] = flipped[3, ::-1]
    degenerate[0, 1] = degenerate[0, 0]
    outside[0, 0] = len(V)
    for Tk, msg in ((T[:-1], "open"), (flipped, "consistently oriented"), (degenerate, "zero area"), (outside, "out of range")):
        assert build(V, Tk) != 0 and msg in lib.tlfea_last_error().decode(), msg
    # still usable: the resting scene reaches the weight
    for _ in range(40):
        s.Solve()
    r, _ = d.GetFieldObstacleResultant(0)
    assert abs(r[2] - mass.sum() * G) <= 1e-8 * mass.sum() * G
    del s
    d.Destroy()


# ---- 8. the builder on the device ---------------------------------------------------------------------------------------------
LO, HI = np.array([-0.2, -0.15, -0.1]), np.array([0.25, 0.2, 0.15])
obs_mod = __import__("importlib").import_module(tl.__name__ + ".obstacles")
TILE = 128                                                             # kSdfTile of csrc/tlfea_internal.h


@pytest.mark.parametrize("sub", (1, 3, 4, 6))
def test_builder_against_the_box_distance(sub):
    """12 sub^2 triangles: 12; 108, below the LDS tile of 128; 192, not a multiple of it; 432, over three tiles"""
    V, T = fnp.box_triangles(LO, HI, sub)
    assert len(T) == {1: 12, 3: 108, 4: 192, 6: 432}[sub]
    assert (len(T) < TILE) == (sub in (1, 3)) and (sub != 4 or len(T) % TILE) and (sub != 6 or len(T) > 3 * TILE)
    shape, origin, spacing = (9, 8, 7), LO - 0.237, 0.113              # no sample lies on the surface
    S = obs_mod.sdf_from_triangles(V, T, shape, origin, spacing)
    assert S.shape == (7, 8, 9)
    ref = fnp.box_distance(fnp.sample(lambda x: x, shape, origin, spacing), LO, HI)
    assert np.abs(ref).min() > 1e-3 and (ref < 0).sum() > 10 and (ref > 0).any()
    assert np.array_equal(np.sign(S), np.sign(ref))
    err = np.abs(S - ref).max() / np.linalg.norm(HI - LO)
    print("builder", sub, err)
    assert err <= 1e-13
    assert np.array_equal(S, obs_mod.sdf_from_triangles(V, T, shape, origin, spacing))
    assert np.array_equal(np.sign(S), np.sign(obs_mod.sdf_from_triangles(V, T[:, ::-1], shape, origin, spacing)))


def test_builder_on_the_sphere_mesh_boundary():
    _, X = tl.mesh_utils.FEAT10_read_nodes(os.path.join(MESHES, "sphere.1.node"))
    _, conn = tl.mesh_utils.FEAT10_read_elements(os.path.join(MESHES, "sphere.1.ele"))
    d = make_gpu(X, conn, SOFT)
    V, T = d.GetBoundaryTriangles()
    assert fnp.check_closed(V, T) == "" and len(T) == 4 * len(d.GetBoundaryFaces().elem)
    Vc, Tc = d.GetBoundaryTriangles(current=True)
    assert np.array_equal(Vc, V) and np.array_equal(Tc, T)
    diam = np.linalg.norm(V.max(axis=0) - V.min(axis=0)) / np.sqrt(3.0)
    shape = (7, 6, 8)
    origin, spacing = V.min(axis=0) - 0.07 * diam, 1.14 * diam / 5.0
    S = obs_mod.sdf_from_triangles(V, T, shape, origin, spacing)
    ref = fnp.sdf_grid(V, T, shape, origin, spacing)
    assert (ref < 0).sum() >= 8 and (ref > 0).sum() >= 8
    assert np.array_equal(np.sign(S), np.sign(ref))
    print("sphere.1", len(T), np.abs(S - ref).max() / diam)
    assert np.abs(S - ref).max() <= 1e-12 * diam
    # as an obstacle: the default margin gives a field that passes the closed-shape rule, bitwise the same twice
    f1 = tl.RigidField.from_t10_surface(d, 0.2 * diam, 1e8)
    f2 = tl.RigidField.from_triangles(V, T, 0.2 * diam, 1e8)
    assert fnp.closed_shape_ok(f1.values) and np.array_equal(f1.values, f2.values) and (f1.values < 0).any()
    d.Destroy()


# ---- 9. the driver ------------------------------------------------------------------------------------------------------------
def test_tire_over_cleat_driver(tmp_path):
    import subprocess
    exe = os.path.join(os.path.dirname(MESHES), "..", "..", "total-lagrangian-fea_amd", "host", "test_tire_over_cleat")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    foot = tmp_path / "footprint.csv"
    p = subprocess.run(["timeout", "-k", "10", "300", exe, "--mesh_dir=" + MESHES, "--footprint_path=" + str(foot),
                        "--travel=1.2e-3", "18"], capture_output=True, text=True, timeout=320)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    print(p.stdout[-3000:])
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("step ")]
    assert len(rows) == 18
    col = {name: np.array([float(r[r.index(name) + 1]) for r in rows])
           for name in ("cleat_x", "floor_force", "floor_points", "cleat_force", "cleat_points")}
    assert np.all(col["floor_force"] > 0) and np.all(col["floor_points"] > 0)
    assert np.all(col["cleat_x"][:6] == 0.06) and col["cleat_x"][-1] == 0.0 and np.all(np.diff(col["cleat_x"][5:]) < 0)
    assert not col["cleat_force"][:6].any() and not col["cleat_points"][:6].any()      # before the cleat reaches the tire
    first = int(np.argmax(col["cleat_points"] > 0))
    assert first >= 6 and np.all(col["cleat_force"][first:] > 0) and np.all(col["cleat_points"][first:] > 0)
    pts = np.loadtxt(foot, delimiter=",", skiprows=1)               # x, y, z, gap, pressure
    assert pts.shape[1] == 5 and pts.shape[0] > 0
    hit = pts[pts[:, 4] > 0]
    assert hit.shape[0] > 0 and np.all(np.isfinite(hit)) and np.all(hit[:, 3] < 0)
