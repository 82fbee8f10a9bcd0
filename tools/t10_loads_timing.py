"""Cost of the surface loads on T10 boundary faces (DESIGN 3h') at config C (972 000 T10 tets): the same engine run without
loads and with gravity plus a follower pressure on the whole top face z = lz, each for 20 Newton iterations in bench.py's
sequence without profiling (wall clock per iteration, CG iterations) and 20 with the per-stage hipEvent timers.  The load
kernels run inside the "grad" stage -- the pressure kernel over the loaded faces and the gather every evaluation, the
body-force kernel once -- so their cost is the difference of that stage between the two runs.  It is reported beside the
number of loaded faces and the bytes the pressure kernel moves per face (6 node ids, 6 positions in, 18 force rows out, the
face's pressure) and the gather per node (the constant vector, the total, the gradient read and written, two CSR offsets).
The sequence fixes three Newton iterations per step in both runs, so the change of the Newton count that the missing load
stiffness causes is measured separately: steps solved to convergence, without and with the pressure.

--root runs the same measurement on another checkout of this repository (an earlier commit, for an A/B run in one
session); such a checkout may lack the face loads, so pass --modes none with it.

    python tools/t10_loads_timing.py [--steps 20] [--configs C] [--modes none,loaded] [--root DIR] \\
        | tee profiles/r12_t10_loads_timing.txt"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ELEM = ("residual", "grad", "tangent_blocks", "assemble_rows")
HBM = 6.29e12  # bytes/s: the measured float4-copy rate of one MI355X
GRAVITY, PRESSURE = (0.0, 0.0, -9.81), 1.0e3


def engine(tl, wl, w, loaded):
    d, _ = wl.make_engine(tl, w, with_solver=False)
    n_faces = 0
    if loaded:
        d.SetGravity(GRAVITY)
        t0 = time.perf_counter()
        bf = d.GetBoundaryFaces()
        top = np.nonzero(bf.normal[:, 2] > 0.99)[0]
        d.AddFacePressure(top, PRESSURE)
        n_faces = len(top)
        print(f"boundary faces: {len(bf.elem)} found and {n_faces} loaded in {time.perf_counter() - t0:.2f} s (host, once)",
              flush=True)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(*w["params"]))
    s.AnalyzeHessianSparsity()
    s.SetFixedSparsityPattern(True)
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 50000, 25))
    x0 = w["x0"]
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    return d, s, n_faces


def run(tl, wl, w, loaded, steps):
    d, s, n_faces = engine(tl, wl, w, loaded)
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
    res = d.GetLoadResultant() if hasattr(d, "GetLoadResultant") else None
    del s
    d.Destroy()
    q = lambda a, p: float(np.percentile(a, p))
    return dict(newton_ms=1e3 * np.median(wall), q1_ms=1e3 * q(wall, 25), q3_ms=1e3 * q(wall, 75), elem_ms=np.median(elem),
                grad_ms=np.median(grad), grad_q1=q(grad, 25), grad_q3=q(grad, 75), cg=np.median(cg), resultant=res,
                n_faces=n_faces)


def converged_counts(tl, wl, w, loaded, n_steps=3):
    """Newton and CG iterations of whole steps solved to the workload's tolerance (up to 50 inner iterations)"""
    d, s, _ = engine(tl, wl, w, loaded)
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
    ap.add_argument("--configs", default="C")
    ap.add_argument("--modes", default="none,loaded")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--counts", type=int, default=1, help="0: skip the converged-step counts")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    tl = importlib.import_module("total-lagrangian-fea_amd")
    wl = importlib.import_module("total-lagrangian-fea_amd.workloads")
    if tl.device_count() < 1:
        raise SystemExit("t10_loads_timing.py needs a GPU")
    modes = a.modes.split(",")
    print(f"package: {os.path.dirname(os.path.abspath(tl.__file__))}", flush=True)
    for cfg in a.configs.split(","):
        w = wl.build(cfg)
        E, N = w["conn"].shape[0], w["X"].shape[0]
        res = {}
        for mode in modes:
            r = res[mode] = run(tl, wl, w, mode == "loaded", a.steps)
            print(f"{mode}: config={cfg} elements={E} nodes={N} loaded_faces={r['n_faces']} grad_stage_ms={r['grad_ms']:.3f} "
                  f"(quartiles {r['grad_q1']:.3f} {r['grad_q3']:.3f}) element_stage_ms={r['elem_ms']:.3f} "
                  f"newton_iteration_ms={r['newton_ms']:.3f} (quartiles {r['q1_ms']:.3f} {r['q3_ms']:.3f}) "
                  f"cg_iterations={r['cg']:.0f} load_resultant={r['resultant']} (medians over {a.steps})", flush=True)
        if "none" in res and "loaded" in res:
            n, p = res["none"], res["loaded"]
            d_grad = p["grad_ms"] - n["grad_ms"]
            face_bytes = p["n_faces"] * (6 * 4 + 6 * 24 + 18 * 8 + 8)
            gather_bytes = N * (24 + 24 + 48 + 8) + p["n_faces"] * 6 * (4 + 24)
            moved = face_bytes + gather_bytes
            print(f"loaded-none: config={cfg} load_grad_ms={d_grad:.4f} loaded_faces={p['n_faces']} pressure kernel moves "
                  f"{face_bytes / 1e6:.2f} MB, the gather {gather_bytes / 1e6:.1f} MB: "
                  f"{moved / max(d_grad, 1e-9) / 1e-3 / HBM:.3f} of the copy rate if they were the whole difference; "
                  f"kernels/newton_iteration={d_grad / n['newton_ms']:.4f} "
                  f"newton_iteration {p['newton_ms'] / n['newton_ms']:.3f}x cg_iterations {n['cg']:.0f} -> {p['cg']:.0f}",
                  flush=True)
        if a.counts:
            for mode in modes:
                print(f"converged steps, {mode}: (newton, cg) per step = {converged_counts(tl, wl, w, mode == 'loaded')}",
                      flush=True)
