"""Cost of per-element materials at config C (972 000 T10, SVK): the same engine run three ways --
uniform material, a one-entry table equal to it, and two materials split by halves (x < L/2: the config's SVK,
x > L/2: E / 10, other density and damping) -- each for 20 Newton iterations without profiling (wall clock per
iteration, CG iterations) and 20 with the per-stage hipEvent timers (element stage = residual + gradient + assembly).
Prints one line per mode and the ratios to the uniform run.

    python tools/multimaterial_timing.py [--steps 20] | tee profiles/r05_multimaterial_timing.txt"""
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


def run(w, mode, steps):
    d, s = wl.make_engine_t10(tl, w, with_solver=False)
    m = w["material"]
    E = w["conn"].shape[0]
    if mode != "uniform":
        a = tl.ElementMaterial(E=m["E"], nu=m["nu"], rho0=m["rho0"], eta=m["eta"], lamd=m["lamd"])
        if mode == "one_entry":
            d.SetElementMaterials(np.zeros(E, dtype=np.int32), [a])
        else:
            cx = w["X"][w["conn"][:, :4]].mean(axis=1)[:, 0]
            ids = (cx > 0.5 * w["X"][:, 0].max()).astype(np.int32)
            b = tl.ElementMaterial(E=m["E"] / 10, nu=0.3, rho0=1200.0, eta=1e3, lamd=1e3)
            d.SetElementMaterials(ids, [a, b])
        d.CalcMassMatrix()
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
    elem = []
    for _ in range(steps):
        iteration()
        st = s.GetStageMs(reset=True)
        elem.append(sum(st[name][0] for name in ELEM))
    s.SetProfiling(False)
    del s
    d.Destroy()
    return dict(newton_ms=1e3 * np.median(wall), elem_ms=np.median(elem), cg=np.median(cg))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--config", default="C")
    a = ap.parse_args()
    w = wl.build(a.config)
    res = {}
    for mode in ("uniform", "one_entry", "two_halves"):
        r = res[mode] = run(w, mode, a.steps)
        print(f"{mode}: config={a.config} elements={w['conn'].shape[0]} element_stage_ms={r['elem_ms']:.3f} "
              f"newton_iteration_ms={r['newton_ms']:.3f} cg_iterations={r['cg']:.0f} (medians over {a.steps})", flush=True)
    u = res["uniform"]
    for mode in ("one_entry", "two_halves"):
        r = res[mode]
        print(f"{mode}/uniform: element_stage {r['elem_ms'] / u['elem_ms']:.3f}x newton_iteration "
              f"{r['newton_ms'] / u['newton_ms']:.3f}x", flush=True)
