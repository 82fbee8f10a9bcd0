"""Cost of the distributed loads on ANCF meshes at config D (256 000 ANCF-3443 shells): the same engine run
without loads and with gravity plus a follower pressure on the top face of every element, each for 20 Newton iterations in
bench.py's sequence without profiling (wall clock per iteration, CG iterations) and 20 with the per-stage hipEvent timers.
The load kernels run inside the "grad" stage -- the pressure kernel and the gather every evaluation, the body-force
kernel once -- so their cost is the difference of that stage between the two runs.  The pressure kernel is reported
against the bytes it moves per element (16 coefficient ids and vectors in, 48 force rows out, class, mask and scale).
The sequence fixes three Newton iterations per step in both runs, so the change of the Newton count that the missing load
stiffness causes is measured separately: steps solved to convergence, without and with the pressure.

    python tools/ancf_loads_timing.py [--steps 20] [--configs D] | tee profiles/r11_ancf_loads_timing.txt"""
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
HBM = 6.29e12  # bytes/s: the measured float4-copy rate of one MI355X
GRAVITY, PRESSURE = (0.0, 0.0, -9.81), 1.0e3


def engine(w, loaded):
    d, _ = wl.make_engine(tl, w, with_solver=False)
    if loaded:
        d.SetGravity(GRAVITY)
        d.AddFollowerPressure(1, np.arange(w["conn"].shape[0]), PRESSURE)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(*w["params"]))
    s.AnalyzeHessianSparsity()
    s.SetFixedSparsityPattern(True)
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 50000, 25))
    x0 = w["x0"]
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    return d, s


def run(w, loaded, steps):
    d, s = engine(w, loaded)
    k = [0]

    def iteration():  # bench.py's sequence: a new time step every third Newton iteration
        if k[0] % 3 == 0:
            s.BeginStep()
        k[0] += 1
        return s.NewtonIteration()

    for _ in range(3):
        iteration()
    wall, cg = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        _, it = iteration()
        wall.append(time.perf_counter() - t0)
        cg.append(it)
    s.SetProfiling(True)
    s.GetStageMs(reset=True)
    elem, grad = [], []
    for _ in range(steps):
        iteration()
        st = s.GetStageMs(reset=True)
        elem.append(sum(st[name][0] for name in ELEM))
        grad.append(st["grad"][0])
    s.SetProfiling(False)
    res = d.GetLoadResultant()
    del s
    d.Destroy()
    return dict(newton_ms=1e3 * np.median(wall), spread_ms=1e3 * (np.percentile(wall, 75) - np.percentile(wall, 25)),
                elem_ms=np.median(elem), grad_ms=np.median(grad), cg=np.median(cg), resultant=res)


def converged_counts(w, loaded, n_steps=3):
    """Newton and CG iterations of whole steps solved to the workload's tolerance (up to 50 inner iterations)"""
    d, s = engine(w, loaded)
    prm = list(w["params"])
    prm[5] = 50
    s.SetParameters(tl.SyncedNewtonParams(*prm))
    out = []
    for _ in range(n_steps):
        s.Solve()
        st = s.GetStats()
        out.append((st["newton"], st["pcg_iters"]))
    del s
    d.Destroy()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--configs", default="D")
    a = ap.parse_args()
    if tl.device_count() < 1:
        raise SystemExit("ancf_loads_timing.py needs a GPU")
    for cfg in a.configs.split(","):
        w = wl.build(cfg)
        E = w["conn"].shape[0]
        S = 16 if w["kind"] == 3443 else 8
        res = {}
        for mode in ("none", "loaded"):
            r = res[mode] = run(w, mode == "loaded", a.steps)
            print(f"{mode}: config={cfg} elements={E} grad_stage_ms={r['grad_ms']:.3f} element_stage_ms={r['elem_ms']:.3f} "
                  f"newton_iteration_ms={r['newton_ms']:.3f} (interquartile {r['spread_ms']:.3f}) cg_iterations={r['cg']:.0f} "
                  f"load_resultant={r['resultant']} (medians over {a.steps})", flush=True)
        n, p = res["none"], res["loaded"]
        d_grad = p["grad_ms"] - n["grad_ms"]
        moved = E * (S * 4 + S * 24 + 3 * S * 8 + 4 + 4 + 16)
        print(f"loaded-none: config={cfg} load_grad_ms={d_grad:.3f} (pressure kernel moves {moved / 1e6:.1f} MB: "
              f"{moved / max(d_grad, 1e-9) / 1e-3 / HBM:.3f} of the copy rate if it were the whole difference) "
              f"kernels/newton_iteration={d_grad / n['newton_ms']:.4f} "
              f"newton_iteration {p['newton_ms'] / n['newton_ms']:.3f}x cg_iterations {n['cg']:.0f} -> {p['cg']:.0f}", flush=True)
        for mode in ("none", "loaded"):
            print(f"converged steps, {mode}: (newton, cg) per step = {converged_counts(w, mode == 'loaded')}", flush=True)
