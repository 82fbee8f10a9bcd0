"""Contact step vs Newton step on one GPU, with contact active in every timed step: the sphere drop (two sphere.1
meshes, 512 T10, 3 mm overlap at the start, gravity on the top one) and two config-B boxes (10 368 T10 each) pressed
2 cm face to face.  Prints one line per scene: candidate pairs, valid patches, median contact step
(broadphase + narrowphase + forces + f_ext update; wall clock, the update ends with a stream sync) and median Newton step.

    python tools/contact_timing.py [--reps 20]
Run it under `rocprofv3 --kernel-trace --stats -- python tools/contact_timing.py` for the per-kernel breakdown."""
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
from tests.helpers import MESHES, make_gpu  # noqa: E402


def sphere_scene():
    mm = tl.MeshManager()
    for _ in range(2):
        mm.LoadMesh(os.path.join(MESHES, "sphere.1.node"), os.path.join(MESHES, "sphere.1.ele"))
        mm.LoadScalarFieldFromNpz(mm.GetNumMeshes() - 1, os.path.join(MESHES, "sphere.1.uncompressed.npz"))
    z = mm.GetAllNodes()[:mm.GetMeshInstance(0).num_nodes, 2]
    mm.TranslateMesh(1, 0.0, 0.0, z.max() - z.min() - 3e-3)  # the faceted spheres overlap by 3 mm, node to node
    X = mm.GetAllNodes().copy()
    n0 = mm.GetMeshInstance(0).num_nodes
    fixed = np.where(X[:n0, 2] < X[:n0, 2].mean())[0].astype(np.int32)
    mat = dict(kind="svk", E=4e6, nu=0.3, rho0=3500.0, eta=1e4, lamd=1e4)
    base = np.zeros(X.size)  # the driver's gravity on the top sphere
    base[3 * np.arange(n0, X.shape[0]) + 2] = 3500.0 * 4.0 / 3.0 * np.pi * 0.15 ** 3 / (X.shape[0] - n0) * -9.81
    return mm, X, mm.GetAllElements().copy(), mm.GetAllScalarFields(), mm.GetAllElementMeshIds(), fixed, mat, \
        (1e-8, 0.0, 1e-10, 1e12, 3, 5, 5e-4), base


def boxes_scene():
    Xa, ca = tl.mesh_utils.structured_t10_box(12, 12, 12, 1.0, 1.0, 1.0)
    Xb = Xa.copy()
    Xb[:, 2] += 0.98
    X = np.concatenate([Xa, Xb])
    conn = np.concatenate([ca, ca + Xa.shape[0]]).astype(np.int32)
    k = 1e7
    p = np.concatenate([k * np.minimum.reduce([Xa[:, 2], 1 - Xa[:, 2], Xa[:, 0], 1 - Xa[:, 0], Xa[:, 1], 1 - Xa[:, 1]]),
                        k * np.minimum.reduce([Xb[:, 2] - 0.98, 1.98 - Xb[:, 2], Xb[:, 0], 1 - Xb[:, 0], Xb[:, 1],
                                               1 - Xb[:, 1]])])
    mesh = np.concatenate([np.zeros(len(ca)), np.ones(len(ca))]).astype(np.int32)
    fixed = np.where(X[:, 2] < 1e-12)[0].astype(np.int32)
    return None, X, conn, p, mesh, fixed, wl.material("neo"), (1e-4, 1e-6, 1e-4, 1e14, 5, 10, 1e-3), np.zeros(X.size)


def run(name, scene, reps):
    mm, X, conn, p, mesh, fixed, mat, prm, base = scene
    d = make_gpu(X, conn, mat, fixed, base)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(*prm))
    c = tl.HydroelasticPatchCollisionSystem(mm, X, conn, p, mesh, False)
    c.BindElementData(d)
    c.SetBaseForce(base)
    inp = tl.CollisionSystemInput(d_vel_xyz=s.GetVelocityGuessDevicePtr())
    par = tl.CollisionSystemParams(0.2, 0.8)
    tc, tn, npat = [], [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        c.Step(inp, par)
        c.ApplyToElementData()
        t1 = time.perf_counter()
        s.Solve()
        t2 = time.perf_counter()
        if r >= 2:
            tc.append(t1 - t0)
            tn.append(t2 - t1)
            npat.append(c.GetNumPatches())
    print(f"{name}: elements={conn.shape[0]} pairs={c.GetNumContacts()} patches(min/max over the timed steps)={min(npat)}/{max(npat)} "
          f"contact_step_ms={1e3 * np.median(tc):.3f} newton_step_ms={1e3 * np.median(tn):.3f}", flush=True)
    c.Destroy()
    del s
    d.Destroy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    run("sphere_drop", sphere_scene(), a.reps)
    run("configB_boxes", boxes_scene(), a.reps)
