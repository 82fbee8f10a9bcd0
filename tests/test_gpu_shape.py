"""Shape sensitivities of the implicit Newton step on the GPU: the element kernel and its gather against the
numpy restatement (tests/shape_np.py), the rigid-translation identity on the adjoint step's outputs,
SetReferencePositions against a freshly set-up object, torch.autograd through a rollout over the reference geometry
against central differences of forward rollouts, determinism, the untouched state, the refusals and the taper driver.

Meshes as tests/test_gpu_adjoint.py: cube (6 elements: less than a wavefront), beam_3x2x1 (a partial wavefront), res2
(several wavefronts, more than one 128-thread block, a ragged last block); cube also with its mid-edge nodes moved, so
that the elements are curved and the affine form is off."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from tests import adjoint_np as anp
from tests import shape_np as snp
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_gpu, perturbed_state, tl
from tests.test_gpu_adjoint import (ATOL, H_STEP, REL_TOL, RHO, build, natural, newton, set_table, table_of, tip_load,
                                    tip_nodes)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def curved(X, conn, rel=0.01, seed=3):
    """mid-edge nodes moved by `rel` of their edge's length in a random direction"""
    rng = np.random.default_rng(seed)
    Y = X.copy()
    done = set()
    for k, (i, j) in enumerate(anp.EDGES):
        for e in range(conn.shape[0]):
            m = conn[e, 4 + k]
            if m in done:
                continue
            done.add(m)
            d = rng.normal(size=3)
            Y[m] += rel * np.linalg.norm(X[conn[e, i]] - X[conn[e, j]]) * d / np.linalg.norm(d)
    return Y


def restated(d, kind, theta, rho, w, u):
    """shape_np fed the GPU's own grad N, det J, connectivity and positions"""
    q = tl.quadrature
    gradN, detJ, conn = d.RetrieveDnDuPreToCPU(), d.RetrieveDetJToCPU(), d.RetrieveConnectivityToCPU()
    x = np.stack(d.RetrievePositionToCPU(), axis=1)
    F = anp.deformation_gradients(x, conn, gradN)
    rows = snp.shape_rows(F, None, gradN, detJ, q.tet5pt_weights, conn, w, u,
                          anp.shape_values(q.tet5pt_x, q.tet5pt_y, q.tet5pt_z), kind, theta, rho)
    return snp.scatter(rows, conn, x.shape[0])


# ---- the element kernel and its gather ------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True], ids=["uniform", "table3"])
@pytest.mark.parametrize("kind", ["svk", "mr"])
@pytest.mark.parametrize("mesh", ["cube", "cube_curved", "beam_3x2x1", "res2"])
def test_kernel_against_restatement(mesh, kind, table):
    X, conn = load_mesh(mesh.split("_curved")[0])
    if mesh.endswith("_curved"):
        X = curved(X, conn)
    d = make_gpu(X, conn, MATERIALS[kind])
    E = conn.shape[0]
    mats = table_of(kind) if table else [MATERIALS[kind]]
    theta = np.stack([natural(dict(m, kind=kind)) for m in mats])
    rho = np.array([m["rho0"] for m in mats])
    if table:
        ids = (np.arange(E) % 3).astype(np.int32)
        set_table(d, kind, mats, ids)
        d.CalcMassMatrix()           # the mass term uses the densities the mass matrix was assembled with
        theta, rho = theta[ids], rho[ids]
    else:
        theta, rho = theta[0], rho[0]
    Xp, _ = perturbed_state(X, seed=5, sigma=2e-3)
    d.UpdatePositions(Xp[:, 0], Xp[:, 1], Xp[:, 2])
    rng = np.random.default_rng(17)
    w, u = rng.normal(size=3 * X.shape[0]), rng.normal(size=3 * X.shape[0])
    got = d.ShapeSensitivity(w, u)
    ref = restated(d, kind, theta, rho, w, u)
    gap, big = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{mesh} {kind} {'table' if table else 'uniform'}: X_bar gap {gap:.3e} of {big:.3e} ({gap / big:.2e} relative)")
    assert got.shape == (X.shape[0], 3) and big > 0.0
    assert gap <= 1e-10 * big
    d.Destroy()


def test_u_is_optional_two_calls_are_bitwise_equal_and_bad_sizes_are_refused():
    X, conn = load_mesh("res2")
    m = MATERIALS["mr"]
    d = make_gpu(X, conn, m)
    Xp, _ = perturbed_state(X, seed=8, sigma=2e-3)
    d.UpdatePositions(Xp[:, 0], Xp[:, 1], Xp[:, 2])
    rng = np.random.default_rng(2)
    w, u = rng.normal(size=3 * X.shape[0]), rng.normal(size=3 * X.shape[0])
    no_mass, with_mass = d.ShapeSensitivity(w), d.ShapeSensitivity(w, u)
    ref = restated(d, "mr", natural(m), m["rho0"], w, None)
    big = np.abs(ref).max()
    assert np.abs(no_mass - ref).max() <= 1e-10 * big
    # the mass term is there with u: what u adds is the restatement's mass term, which stands well clear of the bound
    mass = restated(d, "mr", natural(m), m["rho0"], w, u) - ref
    assert np.abs(mass).max() > 100 * 1e-10 * big
    assert np.abs((with_mass - no_mass) - mass).max() <= 2e-10 * big
    assert np.array_equal(no_mass, d.ShapeSensitivity(w, np.zeros_like(w)))    # and adds exact zeros with u = 0
    assert np.array_equal(with_mass, d.ShapeSensitivity(w, u))
    assert np.array_equal(no_mass, d.ShapeSensitivity(w))
    with pytest.raises(ValueError):
        d.ShapeSensitivity(w[:-1])
    with pytest.raises(ValueError):
        d.ShapeSensitivity(w, u[:-3])
    with pytest.raises(ValueError):
        d.SetReferencePositions(X[:-1])
    d.Destroy()


# ---- the rigid-translation identity on the adjoint step's outputs ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["svk", "mr"])
def test_translation_identity_on_the_adjoint_step(kind):
    """Moving X, x_prev and the targets by one vector c leaves g and v unchanged, moves x by c and leaves lambda_new: the
    loss moves by sum_b xbar_b . c.  So sum X_bar + sum x_prev_bar + sum t_bar - sum xbar = 0 (tests/test_shape_np.py).
    x_prev_bar is formed as x_t - (v_t - M w / h) / h, which takes H w = v_t for granted, so the solve's residual
    (at most 10 REL_TOL ||v_t||_2, tests/test_gpu_adjoint.py) enters through 1 / h: at most 10 REL_TOL sqrt(3N) of the
    terms' magnitudes, beside the 1e-13 of the sums' own rounding."""
    X, conn, fixed, d = build(kind=kind, gravity=True)
    s = newton(d)
    rng = np.random.default_rng(23)
    n, nc = 3 * X.shape[0], d.get_n_constraint()
    v0 = rng.normal(0.0, 0.05, n)
    s.SetVelocity(v0, v0)
    s.Solve()
    assert s.GetStats()["outer"] == 1 and s.GetStats()["norm_g"] < ATOL
    xbar, vbar, lambar = rng.normal(size=n), rng.normal(0.0, H_STEP, n), rng.normal(0.0, 1.0 / RHO, nc)
    r = s.AdjointStep(xbar, vbar, lambar, want_shape=True)
    parts = [r.X_bar, r.x_prev, r.targets.reshape(-1, 3), -xbar.reshape(-1, 3)]
    total = sum(a.sum(axis=0) for a in parts)
    mag = sum(np.abs(a).sum(axis=0) for a in parts)
    largest = max(np.abs(a).max() for a in parts)
    print(f"{kind}: translation sum {total}, relative to the largest term {np.abs(total).max() / largest:.3e}, to the sum "
          f"of magnitudes {np.abs(total / mag).max():.3e}")
    assert np.abs(r.X_bar).max() > 0.0
    assert np.all(np.abs(total) <= (10 * REL_TOL * np.sqrt(n) + 1e-13) * mag)
    # the kernel pair on its own with the same w and u gives the same X_bar
    u = (s.RetrieveVelocityToCPU() - v0) / H_STEP - np.tile([0.5, -1.0, -9.81], X.shape[0])
    alone = d.ShapeSensitivity(r.f_ext.reshape(-1), u)
    assert np.abs(alone - r.X_bar).max() <= 1e-12 * np.abs(alone).max()
    del s
    d.Destroy()


# ---- SetReferencePositions against a fresh object ---------------------------------------------------------------------------
def moved_reference(X, conn):
    """a straight-sided geometry away from X: stretched, sheared and with its vertices moved a little"""
    rng = np.random.default_rng(13)
    A = np.array([[1.05, 0.03, 0.0], [0.0, 0.93, 0.02], [0.04, 0.0, 1.1]])
    return snp.straight_sided(X @ A.T + rng.normal(0.0, 5e-3, X.shape), conn)


def one_step(d, s, Xr):
    d.UpdatePositions(Xr[:, 0], Xr[:, 1], Xr[:, 2])
    d.UpdateConstraintTargets(Xr[:, 0], Xr[:, 1], Xr[:, 2])
    z = np.zeros(3 * Xr.shape[0])
    s.SetVelocity(z, z)
    s.SetLambda(np.zeros(d.get_n_constraint()))
    s.Solve()
    return np.stack(d.RetrievePositionToCPU(), axis=1)


@pytest.mark.parametrize("table", [False, True], ids=["uniform", "table2"])
def test_set_reference_positions_equals_a_fresh_object(table):
    X, conn = load_mesh("beam_3x2x1")
    fixed, f_ext, m = fixed_x0(X), tip_load(X), MATERIALS["svk"]
    Xr = moved_reference(X, conn)
    E = conn.shape[0]

    def make(X0):
        d = make_gpu(X0, conn, m, fixed, f_ext)
        if table:
            set_table(d, "svk", table_of("svk")[:2], (np.arange(E) >= E // 2).astype(np.int32))
            d.CalcMassMatrix()
        d.SetGravity([0.0, 0.0, -9.81])
        return d, newton(d)
    a, sa = make(X)
    one_step(a, sa, X)             # the solver's caches are those of the old geometry when the reference moves
    a.SetReferencePositions(Xr)
    b, sb = make(Xr)
    pairs = [("grad N", a.RetrieveDnDuPreToCPU(), b.RetrieveDnDuPreToCPU()), ("det J", a.RetrieveDetJToCPU(), b.RetrieveDetJToCPU()),
             ("mass values", a.RetrieveMassCSRToCPU()[2], b.RetrieveMassCSRToCPU()[2]),
             ("positions after one step", one_step(a, sa, Xr) - Xr, one_step(b, sb, Xr) - Xr)]
    bad = []
    for name, got, ref in pairs:
        gap = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"{'table' if table else 'uniform'} {name}: relative gap {gap:.3e}, bitwise equal: {np.array_equal(got, ref)}")
        if not gap <= 1e-10:
            bad.append((name, gap))
    assert not bad, bad
    assert np.abs(pairs[3][2]).max() > 1e-5       # the step moved the beam
    del sa, sb
    a.Destroy()
    b.Destroy()


def test_an_inverted_element_is_refused_and_the_old_geometry_still_solves():
    X, conn = load_mesh("beam_3x2x1")
    fixed = fixed_x0(X)
    d = make_gpu(X, conn, MATERIALS["svk"], fixed, tip_load(X))
    s = newton(d)
    before = (d.RetrieveDnDuPreToCPU(), d.RetrieveDetJToCPU(), d.RetrieveMassCSRToCPU()[2])
    x1 = one_step(d, s, X)
    bad = X.copy()
    e = conn.shape[0] // 2
    # vertex 0 of one element pushed through its opposite face, the mid-edge nodes following it
    bad[conn[e, 0]] += 2.5 * (X[conn[e, 1:4]].mean(axis=0) - X[conn[e, 0]])
    bad = snp.straight_sided(bad, conn)
    with pytest.raises(tl.TlfeaError, match="inverted"):
        d.SetReferencePositions(bad)
    after = (d.RetrieveDnDuPreToCPU(), d.RetrieveDetJToCPU(), d.RetrieveMassCSRToCPU()[2])
    assert all(np.array_equal(p, q) for p, q in zip(before, after))
    assert np.array_equal(np.asarray(d._X0), X)
    x2 = one_step(d, s, X)     # the same step again (the linear solver starts warm: not bitwise)
    assert np.abs(x2 - x1).max() <= 1e-10 * np.abs(x1 - X).max()
    del s
    d.Destroy()


# ---- torch.autograd through a rollout over the reference geometry ----------------------------------------------------------
def fd_lines(lines):
    """TLFEA_SHAPE_FD_OUT=<file> also appends the lines to that file (how profiles/shape_fd.txt is written)"""
    out = os.environ.get("TLFEA_SHAPE_FD_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("through_vertices", [True, False], ids=["vertices_through_straight_sided", "all_nodes"])
def test_rollout_gradients_over_the_reference_against_central_differences(through_vertices):
    """3 steps on the clamped beam_3x2x1 from rest at x_0 = X with the clamped nodes' targets on X; loss = mean tip z +
    1e-4 |v|^2.  Two directions of X: the vertices alone through straight_sided (the mid-edge nodes follow), and every
    node on its own.  Central differences with eps = 1e-4 of the mesh extent, the direction scaled to a largest entry of 1;
    bound 1e-5 relative (tests/test_gpu_adjoint.py's).  Measured: 5.2e-12 and 1.4e-10 (profiles/shape_fd.txt)."""
    import torch
    diff = importlib.import_module("total-lagrangian-fea_amd.differentiable")
    X, conn, fixed, d = build(gravity=True)
    s = newton(d)
    N, tip = X.shape[0], tip_nodes(X)
    f_ext = torch.tensor(tip_load(X).reshape(N, 3))
    gravity = torch.tensor([0.0, 0.0, -9.81], dtype=torch.float64)
    fx = torch.as_tensor(np.asarray(fixed, dtype=np.int64))

    def loss_of(Xn, grad):
        P = torch.tensor(Xn, dtype=torch.float64, requires_grad=grad)
        R = diff.straight_sided(P, conn) if through_vertices else P
        state = (R, torch.zeros((N, 3), dtype=torch.float64), torch.zeros(3 * len(fixed), dtype=torch.float64))
        x, v, _ = diff.rollout(s, d, state, 3, f_ext=f_ext, targets=R[fx], gravity=gravity, reference=R)
        return x[tip, 2].mean() + 1e-4 * (v * v).sum(), P
    rng = np.random.default_rng(43 if through_vertices else 44)
    eps = 1e-4 * np.ptp(X, axis=0).max()
    name = "vertices through straight_sided" if through_vertices else "all nodes"
    direction = rng.normal(size=X.shape)
    direction /= np.abs(direction).max()
    loss, P = loss_of(X, True)
    loss.backward()
    grad = P.grad.numpy()
    adj = float((grad * direction).sum())
    fd = (float(loss_of(X + eps * direction, False)[0]) - float(loss_of(X - eps * direction, False)[0])) / (2.0 * eps)
    gap = abs(adj - fd) / abs(fd)
    line = (f"beam_3x2x1 d loss / d X ({name}, random direction): autograd {adj:+.12e} central difference {fd:+.12e} "
            f"relative gap {gap:.3e}")
    print(line)
    fd_lines([line])
    if through_vertices:   # the mid-edge rows of the parameter are not read
        mid = np.setdiff1d(np.arange(N), np.unique(conn[:, :4]))
        assert np.all(grad[mid] == 0.0) and np.abs(grad).max() > 0.0
    # the nine-argument form still runs, on a reference that was moved and put back
    d.SetReferencePositions(X)
    x9, _, _ = diff.rollout(s, d, (torch.tensor(X), torch.zeros((N, 3), dtype=torch.float64),
                                   torch.zeros(3 * len(fixed), dtype=torch.float64)), 1, f_ext=f_ext)
    assert np.array_equal(np.asarray(d._X0), X) and np.isfinite(x9.numpy()).all()
    del s
    d.Destroy()
    assert gap <= 1e-5, line


# ---- refusals and untouched paths --------------------------------------------------------------------------------------------
def test_new_refusals_name_their_cause_and_the_old_entry_points_still_work():
    for what, word in (("plane", "obstacle"), ("traction", "traction")):
        X, conn, fixed, d = build(plane=(what == "plane"), gravity=True)
        if what == "traction":
            bf = d.GetBoundaryFaces()
            d.AddFaceTraction(np.nonzero(bf.normal[:, 2] > 0.99)[0], [0.0, 0.0, -1e3])
        s = newton(d)
        s.Solve()
        n = 3 * X.shape[0]
        plain = s.AdjointStep(np.ones(n))                     # without X_bar nothing changes
        assert plain.X_bar is None and np.isfinite(plain.f_ext).all()
        with pytest.raises(tl.TlfeaError, match=word):
            s.AdjointStep(np.ones(n), want_shape=True)
        again = s.AdjointStep(np.ones(n))
        assert np.array_equal(plain.f_ext, again.f_ext) and np.array_equal(plain.x_prev, again.x_prev)
        # the kernel pair alone and a moved reference are not refused: the loads follow the new geometry
        assert np.isfinite(d.ShapeSensitivity(plain.f_ext.reshape(-1))).all()
        d.SetReferencePositions(X * 1.01)
        d.SetReferencePositions(X)
        s.Solve()
        del s
        d.Destroy()


def test_refusal_of_an_ancf_handle():
    from tests.test_gpu_ancf import SVK, beam_problem, make_pair
    _, d = make_pair(beam_problem(), SVK)
    nc = d.get_n_coef()
    out = np.zeros(3 * nc)
    lib = tl.load_library()
    dp = importlib.import_module("total-lagrangian-fea_amd.binding").dp
    assert lib.tlfea_t10_shape_sensitivity(d._h, dp(out), None, dp(out)) != 0
    assert b"ANCF" in lib.tlfea_last_error()
    x = np.zeros(nc)
    assert lib.tlfea_t10_set_reference_positions(d._h, dp(x), dp(x), dp(x), nc) != 0
    assert b"ANCF" in lib.tlfea_last_error()
    assert lib.tlfea_t10_time_shape_kernels(d._h, 1, dp(out)) != 0
    assert b"ANCF" in lib.tlfea_last_error()
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    with pytest.raises(tl.TlfeaError, match="ANCF"):
        s.AdjointStep(np.ones(3 * nc), want_shape=True)
    del s
    d.Destroy()


@pytest.mark.parametrize("method", [0, 1], ids=["cg", "direct"])
def test_two_calls_are_bitwise_equal_and_the_trajectory_is_untouched(method):
    rng = np.random.default_rng(31)
    out = []
    for with_adjoint in (False, True):
        X, conn, fixed, d = build(gravity=True, table=True)
        s = newton(d, method)
        n, nc = 3 * X.shape[0], d.get_n_constraint()
        xbar, vbar, lambar = rng.normal(size=n), rng.normal(size=n), rng.normal(0.0, 1.0 / RHO, nc)
        traj = []
        for _ in range(3):
            s.Solve()
            if with_adjoint:
                a, b = (s.AdjointStep(xbar, vbar, lambar, per_element=True, want_shape=True) for _ in range(2))
                for f in ("X_bar", "f_ext", "v_prev", "x_prev", "lam_in", "targets", "gravity", "per_material", "per_element"):
                    assert np.array_equal(getattr(a, f), getattr(b, f)), f
                assert np.abs(a.X_bar).max() > 0.0
                c = s.AdjointStep(xbar, vbar, lambar, per_element=True)   # X_bar changes no other output's bits
                for f in ("f_ext", "v_prev", "x_prev", "lam_in", "targets", "gravity", "per_material", "per_element"):
                    assert np.array_equal(getattr(a, f), getattr(c, f)), f
            traj.append((np.stack(d.RetrievePositionToCPU()), s.RetrieveVelocityToCPU(), s.RetrieveLambdaToCPU(),
                         s.GetStats()["pcg_iters"]))
        out.append(traj)
        del s
        d.Destroy()
    for plain, adj in zip(*out):
        for p, q in zip(plain[:3], adj[:3]):
            assert np.array_equal(p, q)
        assert plain[3] == adj[3]


# ---- the taper driver ---------------------------------------------------------------------------------------------------------
def run_driver(*args):
    exe = os.path.join(ROOT, "total-lagrangian-fea_amd", "host", "test_beam_taper")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is missing: build() compiles the host drivers")
    return subprocess.run([exe, "--mesh_dir=" + os.path.join(ROOT, "tests", "golden", "meshes"), *args],
                          capture_output=True, text=True, timeout=300)


def test_driver_recovers_the_scale():
    r = run_driver()
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    its = [ln for ln in r.stdout.splitlines() if ln.startswith("iterate")]
    assert "recovered in" in r.stdout and len(its) - 1 <= 8
    assert float(its[-1].split("=")[-1]) <= 1e-6
    assert abs(float(its[0].split("=")[-1]) - 0.2) < 1e-12      # it started 20 % off


def test_driver_with_a_wrong_derivative_does_not_get_there():
    r = run_driver("--wrong_derivative=1")
    assert r.returncode == 2 and "not recovered" in r.stdout, r.stdout + r.stderr
