"""Cost of the rigid obstacles on ANCF meshes (DESIGN 3e') at config D (256 000 ANCF-3443 shells): the same engine run
without and with a slightly tilted, very soft floor (1e3 Pa/m, up to 5 mm deep: soft enough that the unloaded plate is
not thrown off it during the run) under the half x > x_c of the plate, each for 20 Newton iterations in bench.py's
sequence without profiling (wall clock per iteration, CG iterations) and 20 with the per-stage hipEvent timers.  The
contact kernels run inside two stages -- the points and gather kernels in "grad", the tangent kernel in "assemble_rows"
-- so their cost is the difference of those stages between the two runs.  The tangent kernel is reported against the
bytes it moves (136 pairs x 72 bytes each way plus 1.5 kB of C_p per touched shell).  The sequence fixes three Newton
iterations per step in both runs; touched elements are counted after the warm-up and at the end.
A third run adds a field obstacle far above the plate beside the floor (DESIGN 3e''): it covers no point, so the floor's
work is the same, and the difference to the second run is the cost of the kernels' field instantiations.

    python tools/ancf_obstacle_timing.py [--steps 20] [--configs D] | tee profiles/r10_ancf_obstacle_timing.txt"""
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


def run(w, with_floor, steps, with_field=False):
    d, _ = wl.make_engine(tl, w, with_solver=False)
    touched = 0
    if with_floor:
        L, W, H = w["dims"]
        xc = 0.5 * w["X"][0::4, 0].max()
        n = np.array([-2e-4, 0.0, 1.0])
        d.SetRigidObstacles([tl.RigidPlane([xc, 0.0, -H / 2], n / np.linalg.norm(n), 1e3)])
    if with_field:
        # a field far above the plate beside the floor (DESIGN 3e''): it touches nothing, so the floor's work is the same,
        # but the list holds a field and the launches take the kernels' field instantiations
        zc = w["X"][0::4, 2].max() + 100.0
        d.SetFieldObstacles([tl.RigidField.from_function(lambda p: np.linalg.norm(p - [xc, 0.0, zc], axis=-1) - 1.0,
                                                         [xc - 3.0, -3.0, zc - 3.0], [xc + 3.0, 3.0, zc + 3.0], 0.5, 1e3)])
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

    def count_touched():
        return int(np.count_nonzero(d.RetrieveContactPointsToCPU()[:, :, 4].max(axis=1) > 0)) if with_floor else 0

    touched0 = count_touched()
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
    active = 0
    if with_floor:
        active = d.GetObstacleResultant(0)[1]
        touched = count_touched()
    del s
    d.Destroy()
    return dict(newton_ms=1e3 * np.median(wall), elem_ms=np.median(elem), grad_ms=np.median(grad),
                asm_ms=np.median(asm), cg=np.median(cg), touched=touched, touched0=touched0, active=active)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--configs", default="D")
    a = ap.parse_args()
    if tl.device_count() < 1:
        raise SystemExit("ancf_obstacle_timing.py needs a GPU")
    for cfg in a.configs.split(","):
        w = wl.build(cfg)
        E = w["conn"].shape[0]
        S = 16 if w["kind"] == 3443 else 8
        res = {}
        modes = ("none", "floor") + (("floor+field",) if hasattr(tl, "RigidField") else ())
        for mode in modes:
            r = res[mode] = run(w, mode != "none", a.steps, mode == "floor+field")
            print(f"{mode}: config={cfg} elements={E} touched_elements={r['touched0']}..{r['touched']} "
                  f"(after warm-up..at the end) points_in_contact={r['active']} "
                  f"grad_stage_ms={r['grad_ms']:.3f} assembly_stage_ms={r['asm_ms']:.3f} element_stage_ms={r['elem_ms']:.3f} "
                  f"newton_iteration_ms={r['newton_ms']:.3f} cg_iterations={r['cg']:.0f} newton_iterations_per_step=3 "
                  f"(medians over {a.steps})", flush=True)
        n, p = res["none"], res["floor"]
        d_grad, d_asm = p["grad_ms"] - n["grad_ms"], p["asm_ms"] - n["asm_ms"]
        n_t = min(p["touched"], p["touched0"])
        kbuf = n_t * (S * (S + 1) // 2) * 72 * 2 + n_t * 32 * 48
        pts = E * (S * 4 + 2 * S * 24 + 32 * 8 + S * 24 + 4) + n_t * 32 * 48
        print(f"floor-none: config={cfg} contact_grad_ms={d_grad:.3f} (points kernel moves {pts / 1e6:.1f} MB: "
              f"{pts / max(d_grad, 1e-9) / 1e-3 / HBM:.3f} of the copy rate) contact_tangent_ms={d_asm:.3f} "
              f"(Kbuf read-modify-write and C_p read {kbuf / 1e6:.1f} MB: {kbuf / max(d_asm, 1e-9) / 1e-3 / HBM:.3f} of the copy rate) "
              f"kernels/newton_iteration={(d_grad + d_asm) / n['newton_ms']:.4f} "
              f"newton_iteration {p['newton_ms'] / n['newton_ms']:.3f}x cg_iterations {n['cg']:.0f} -> {p['cg']:.0f}",
              flush=True)
        if "floor+field" in res:
            f = res["floor+field"]
            print(f"floor+field - floor: config={cfg} grad_stage_ms {f['grad_ms'] - p['grad_ms']:+.3f} (the points kernel's field "
                  f"instantiation, 3 waves per SIMD instead of 4) assembly_stage_ms {f['asm_ms'] - p['asm_ms']:+.3f} "
                  f"newton_iteration {f['newton_ms'] / p['newton_ms']:.4f}x", flush=True)
