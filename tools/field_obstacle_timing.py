"""Measurements of the field obstacles (DESIGN 3e'').

    python tools/field_obstacle_timing.py timing [--steps 20] [--config C]   per-iteration cost at config C: no obstacles,
        a floor plane 1e-4 of the height above the bottom face, and the plane plus a field box under the first third of the
        bottom face; medians and quartiles of the Newton iteration and of the grad stage (the obstacle kernel runs in it).
        On a tree without field obstacles the third case is skipped, so the same file times the parent commit.
    python tools/field_obstacle_timing.py builder      (sample, triangle) pairs per second of tlfea_sdf_from_triangles on
        the boundary of sphere.1 at 64^3 and 128^3
    python tools/field_obstacle_timing.py sphere       a block pressed to three depths onto the field built from sphere.1's
        boundary and onto the RigidSphere of the same radius: resultants side by side (faceting + interpolation)
    python tools/field_obstacle_timing.py newton       Newton iterations of the resting steps with a plane and with a field"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
tl = importlib.import_module("total-lagrangian-fea_amd")
wl = importlib.import_module("total-lagrangian-fea_amd.workloads")
MESHES = os.path.join(ROOT, "tests", "golden", "meshes")


def box_distance(p, lo, hi):
    c, hw = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q = np.abs(p - c) - hw
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(np.max(q, axis=-1), 0.0)


def quartiles(v):
    return np.percentile(v, [25, 50, 75])


def run(w, mode, steps):
    d, _ = wl.make_engine_t10(tl, w, with_solver=False)
    X = w["X"]
    lo, hi = X.min(axis=0), X.max(axis=0)
    top = lo[2] + 1e-4 * (hi[2] - lo[2])
    if mode != "none":
        d.SetRigidObstacles([tl.RigidPlane([0, 0, top], [0, 0, 1], 1e10)])
    if mode == "plane+field":
        sp = (hi[0] - lo[0]) / 48.0
        blo = np.array([lo[0] - 4 * sp, lo[1] - 4 * sp, top - 6 * sp])
        bhi = np.array([lo[0] + (hi[0] - lo[0]) / 3.0, hi[1] + 4 * sp, top])
        d.SetFieldObstacles([tl.RigidField.from_function(lambda p: box_distance(p, blo, bhi), blo - 3 * sp, bhi + 3 * sp, sp,
                                                         1e10)])
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(*w["params"]))
    s.AnalyzeHessianSparsity()
    s.SetFixedSparsityPattern(True)
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 50000, 25))
    x0 = w["x0"]
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    k = [0]

    def iteration():  # bench.py's sequence: a new time step every third Newton iteration
        if k[0] % 3 == 0:
            s.BeginStep()
        k[0] += 1
        return s.NewtonIteration()

    for _ in range(3):
        iteration()
    wall = []
    for _ in range(steps):
        t0 = time.perf_counter()
        iteration()
        wall.append(1e3 * (time.perf_counter() - t0))
    s.SetProfiling(True)
    s.GetStageMs(reset=True)
    grad = []
    for _ in range(steps):
        iteration()
        grad.append(s.GetStageMs(reset=True)["grad"][0])
    s.SetProfiling(False)
    act = [d.GetObstacleResultant(0)[1] if mode != "none" else 0, d.GetFieldObstacleResultant(0)[1] if mode == "plane+field" else 0]
    del s
    d.Destroy()
    return quartiles(wall), quartiles(grad), act


def timing(a):
    w = wl.build(a.config)
    modes = ["none", "plane"] + (["plane+field"] if hasattr(tl, "RigidField") else [])
    res = {}
    for mode in modes:
        res[mode] = run(w, mode, a.steps)
        wq, gq, act = res[mode]
        print(f"{mode}: config={a.config} elements={w['conn'].shape[0]} contacts plane={act[0]} field={act[1]} "
              f"newton_iteration_ms q25/q50/q75 = {wq[0]:.3f}/{wq[1]:.3f}/{wq[2]:.3f} "
              f"grad_stage_ms q25/q50/q75 = {gq[0]:.4f}/{gq[1]:.4f}/{gq[2]:.4f} (over {a.steps})", flush=True)
    if "plane+field" in res:
        print(f"field - plane: grad_stage_ms {res['plane+field'][1][1] - res['plane'][1][1]:.4f} "
              f"newton_iteration {res['plane+field'][0][1] / res['plane'][0][1]:.4f}x", flush=True)


def sphere_surface():
    _, X = tl.mesh_utils.FEAT10_read_nodes(os.path.join(MESHES, "sphere.1.node"))
    _, conn = tl.mesh_utils.FEAT10_read_elements(os.path.join(MESHES, "sphere.1.ele"))
    q = tl.quadrature
    d = tl.GPU_FEAT10_Data(conn.shape[0], X.shape[0])
    d.Initialize()
    d.Setup(q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights, X[:, 0], X[:, 1], X[:, 2], conn)
    V, T = d.GetBoundaryTriangles()
    d.Destroy()
    return V, T


def builder(a):
    obs = importlib.import_module("total-lagrangian-fea_amd.obstacles")
    V, T = sphere_surface()
    lo, hi = V.min(axis=0), V.max(axis=0)
    for n in (64, 128):
        sp = 1.2 * (hi - lo).max() / (n - 1)
        org = 0.5 * (lo + hi) - 0.5 * (n - 1) * sp
        obs.sdf_from_triangles(V, T, (8, 8, 8), org, sp)           # warm-up
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            S = obs.sdf_from_triangles(V, T, (n, n, n), org, sp)
            t.append(time.perf_counter() - t0)
        pairs = n ** 3 * len(T)
        print(f"builder: grid={n}^3 triangles={len(T)} pairs={pairs:.3e} seconds(min of 3, with copies)={min(t):.4f} "
              f"pairs_per_second={pairs / min(t):.3e} inside={int((S < 0).sum())}", flush=True)


def t10_body(X, conn, gravity=True):
    q = tl.quadrature
    d = tl.GPU_FEAT10_Data(conn.shape[0], X.shape[0])
    d.Initialize()
    d.Setup(q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights, X[:, 0], X[:, 1], X[:, 2], conn)
    d.SetDensity(1000.0)
    d.SetDamping(0.0, 0.0)
    d.SetSVK(1e7, 0.3)
    d.CalcDnDuPre()
    d.CalcMassMatrix()
    off, _, val = d.RetrieveMassCSRToCPU()
    mass = np.add.reduceat(val, off[:-1])
    if gravity:
        d.SetExternalForce((mass[:, None] * np.array([0.0, 0.0, -9.81])[None, :]).reshape(-1))
    return d, mass.sum() * 9.81


def newton_solver(d, h):
    s = tl.SyncedNewtonSolver(d, 0)
    s.SetParameters(tl.SyncedNewtonParams(1e-7, 0.0, 1e-6, 1e14, 1, 40, h))
    s.SetLinSolveOpts(tl.LinSolveOpts(rel_tol=1e-13, max_iter=50000))
    return s


def sphere(a):
    """One gradient evaluation per depth: the bottom face of a 0.5 x 0.5 x 0.25 block (8 x 8 x 2 cells) pushed `depth` into
    the top of the sphere, once as the field built from sphere.1's boundary (spacing R / 16), once as the RigidSphere."""
    V, T = sphere_surface()
    c = 0.5 * (V.min(axis=0) + V.max(axis=0))
    R = float(np.linalg.norm(V - c, axis=1).max())
    X, conn = tl.mesh_utils.structured_t10_box(8, 8, 2, 0.5, 0.5, 0.25)
    for depth in (0.02 * R, 0.05 * R, 0.1 * R):
        shift = np.array([0.25, 0.25, -R + depth]) - c
        fld = tl.RigidField.from_triangles(V + shift, T, R / 16.0, 1e9)
        ana = tl.RigidSphere(c + shift, R, 1e9)
        for name, o, is_field in (("field(sphere.1 boundary)", fld, True), ("RigidSphere", ana, False)):
            d, _ = t10_body(X, conn, gravity=False)
            (d.SetFieldObstacles if is_field else d.SetRigidObstacles)([o])
            s = newton_solver(d, 1e-2)
            s.AnalyzeHessianSparsity()
            s.BeginStep()
            s.EvalGradient()
            r, n = (d.GetFieldObstacleResultant if is_field else d.GetObstacleResultant)(0)
            del s
            d.Destroy()
            print(f"sphere: {name} radius={R:.4f} depth={depth:.5f} grid={fld.shape} resultant={r} nodes_in_contact={n}",
                  flush=True)


def newton(a):
    """The resting step of the tests (beam_3x2x1 under gravity, h = 0.05, 40 steps) on a plane and on the flat top of a
    field box: Newton iterations per step and the resultant against the weight."""
    _, X = tl.mesh_utils.FEAT10_read_nodes(os.path.join(MESHES, "beam_3x2x1.1.node"))
    _, conn = tl.mesh_utils.FEAT10_read_elements(os.path.join(MESHES, "beam_3x2x1.1.ele"))
    lo, hi = np.array([-2.5, -2.5, -1.5]), np.array([5.5, 4.5, 0.0])
    fld = tl.RigidField.from_function(lambda p: box_distance(p, lo, hi), lo - 1.5, hi + 1.5, 0.5, 1e8)
    for name, o, is_field in (("plane", tl.RigidPlane([0, 0, 0], [0, 0, 1], 1e8), False), ("field box", fld, True)):
        d, W = t10_body(X, conn)
        (d.SetFieldObstacles if is_field else d.SetRigidObstacles)([o])
        s = newton_solver(d, 0.05)
        iters = []
        for _ in range(40):
            s.Solve()
            iters.append(int(s.GetStats()["newton"]))
        r, n = (d.GetFieldObstacleResultant if is_field else d.GetObstacleResultant)(0)
        del s
        d.Destroy()
        print(f"newton: {name} resultant_z={r[2]:.6f} weight={W:.6f} nodes_in_contact={n} newton_iterations_per_step={iters}",
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "builder", "sphere", "newton"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--config", default="C")
    a = ap.parse_args()
    {"timing": timing, "builder": builder, "sphere": sphere, "newton": newton}[a.what](a)
