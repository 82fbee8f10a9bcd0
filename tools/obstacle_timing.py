"""Cost of the rigid obstacles at config C (972 000 T10, SVK) and config B: the same engine run without and
with a half-space 1e-4 of the height above the bottom face z = 0 (all of its nodes in contact), each for 20 Newton iterations without profiling (wall clock per
iteration, CG iterations) and 20 with the per-stage hipEvent timers.  The obstacle kernels run inside two stages --
obstacle_grad_kernel in "grad", obstacle_hessian_kernel in "assemble_rows" -- so their cost is the difference of those
stages between the two runs; the element stage is residual + gradient + assembly.  Prints one line per run and the
differences.

    python tools/obstacle_timing.py [--steps 20] [--configs C,B] | tee profiles/r06_obstacle_timing.txt"""
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

ELEM = ("residual", "grad", "tangent_blocks", "assemble_rows")


def run(w, with_plane, steps):
    d, _ = wl.make_engine_t10(tl, w, with_solver=False)
    n_surf = 0
    if with_plane:
        # the plane 1e-4 of the height above z = 0: every node of the bottom face starts in contact
        d.SetRigidObstacles([tl.RigidPlane([0, 0, 1e-4 * w["X"][:, 2].max()], [0, 0, 1], 1e10)])
        n_surf = int(np.count_nonzero(d.GetSurfaceWeights()))
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

    for _ in range(3):  # warm-up: graphs, work lists, the polynomial's bounds
        iteration()
    wall, cg = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        _, it = iteration()
        wall.append(time.perf_counter() - t0)
        cg.append(it)
    s.SetProfiling(True)
    s.GetStageMs(reset=True)
    elem, grad, asm = [], [], []
    for _ in range(steps):
        iteration()
        st = s.GetStageMs(reset=True)
        elem.append(sum(st[name][0] for name in ELEM))
        grad.append(st["grad"][0])
        asm.append(st["assemble_rows"][0])
    s.SetProfiling(False)
    active = d.GetObstacleResultant(0)[1] if with_plane else 0
    del s
    d.Destroy()
    return dict(newton_ms=1e3 * np.median(wall), elem_ms=np.median(elem), grad_ms=np.median(grad),
                asm_ms=np.median(asm), cg=np.median(cg), n_surf=n_surf, active=active)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--configs", default="C,B")
    a = ap.parse_args()
    for cfg in a.configs.split(","):
        w = wl.build(cfg)
        res = {}
        for mode in ("none", "plane"):
            r = res[mode] = run(w, mode == "plane", a.steps)
            print(f"{mode}: config={cfg} elements={w['conn'].shape[0]} surface_nodes={r['n_surf']} contacts={r['active']} "
                  f"grad_stage_ms={r['grad_ms']:.3f} assembly_stage_ms={r['asm_ms']:.3f} element_stage_ms={r['elem_ms']:.3f} "
                  f"newton_iteration_ms={r['newton_ms']:.3f} cg_iterations={r['cg']:.0f} (medians over {a.steps})",
                  flush=True)
        n, p = res["none"], res["plane"]
        kern = (p["grad_ms"] - n["grad_ms"]) + (p["asm_ms"] - n["asm_ms"])
        print(f"plane-none: config={cfg} obstacle_grad_ms={p['grad_ms'] - n['grad_ms']:.3f} "
              f"obstacle_hessian_ms={p['asm_ms'] - n['asm_ms']:.3f} kernels/newton_iteration={kern / n['newton_ms']:.4f} "
              f"element_stage {p['elem_ms'] / n['elem_ms']:.3f}x newton_iteration {p['newton_ms'] / n['newton_ms']:.3f}x "
              f"cg_iterations {n['cg']:.0f} -> {p['cg']:.0f}", flush=True)
