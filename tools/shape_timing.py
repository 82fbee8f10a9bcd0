"""Cost of the shape sensitivities at config B (10 368 T10, neo-Hookean) and config C (972 000 T10, SVK), in
one process per config, by tools/adjoint_timing.py's method: shape_point_kernel, its gather, sens_point_kernel and
stress_point_kernel as medians of 4 x `samples` hipEvent pairs around `reps` back-to-back launches; the adjoint step
(device form, per-material outputs) with and without X_bar as medians of host-clock samples around calls that end in a
device synchronise; and the bytes the element kernels have to move against the measured HBM copy rate.

    python tools/shape_timing.py [--samples 5] [--reps 10] [--configs B,C] | tee profiles/shape_timing.txt"""
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
binding = importlib.import_module("total-lagrangian-fea_amd.binding")

HBM = 6.29e12  # bytes/s: the measured float4-copy rate of one MI355X (8.0e12 is the datasheet figure)


def run(cfg, samples, reps):
    import torch
    w = wl.build(cfg)
    d, s = wl.make_engine_t10(tl, w)
    p = list(w["params"])
    p[4] = 1  # one outer iteration: the step the adjoint differentiates
    p[1] = max(p[1], 1e-6)
    s.SetParameters(tl.SyncedNewtonParams(*p))
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 50000, 25))
    x0 = w["x0"]
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    s.BeginStep()
    for _ in range(3):  # warm-up: buffers, the preconditioner's hierarchy, the captured CG graphs
        s.NewtonIteration()
    E, N = w["conn"].shape[0], w["X"].shape[0]
    # a whole step from the start state again: its Newton loop leaves through inner_rtol of the first ||g||
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    s.SetVelocity(np.zeros(3 * N), np.zeros(3 * N))
    s.Solve()
    st = s.GetStats()
    s.AdjointReady()
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(7)
    n, nc = 3 * N, s.n_constraints
    n_mat, slots = d.MaterialSensitivityShape()
    ins = [torch.randn(n, dtype=torch.float64, generator=gen).to(dev), torch.randn(n, dtype=torch.float64, generator=gen).to(dev),
           (torch.randn(nc, dtype=torch.float64, generator=gen) / p[3]).to(dev), None]
    z = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)  # noqa: E731
    outs = [z(n), z(n), z(n), z(nc), z(nc), z(3), z(n_mat * slots), None]
    X_bar = z(n)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    cin, cout = binding.AdjointInC(*[ptr(t) for t in ins]), binding.AdjointOutC(*[ptr(t) for t in outs])
    torch.cuda.synchronize()
    adj = {}
    for name, xb in (("without", None), ("with", ptr(X_bar))):
        s.AdjointStepDevice(cin, cout, xb)
        ms, its = [], []
        for _ in range(samples):
            t0 = time.perf_counter()
            it, rel = s.AdjointStepDevice(cin, cout, xb)
            ms.append(1e3 * (time.perf_counter() - t0))
            its.append(it)
        adj[name] = (np.median(ms), sorted(set(its)), rel)
    d.TimeShapeKernels(reps)
    shape = np.median([d.TimeShapeKernels(reps) for _ in range(4 * samples)], axis=0)
    d.TimeSensitivityKernels(reps)
    sens = np.median([d.TimeSensitivityKernels(reps) for _ in range(4 * samples)], axis=0)
    d.TimeStressKernels(None, False, reps)
    stress = np.median([d.TimeStressKernels(None, False, reps) for _ in range(4 * samples)], axis=0)
    # bytes each element kernel has to move once: connectivity, 150 gradients, det J, positions; the shape and sensitivity
    # kernels add w and u; the shape kernel stores 30 doubles per element, the sensitivity kernel P + 1, the stress kernel
    # its 10-double record and 4 integrals.  The gather reads the 30 doubles and the incidence (10 ints) per element and
    # stores 3 doubles per node.
    common = E * (10 * 4 + 150 * 8 + 5 * 8) + N * 3 * 8
    b_shape, b_sens, b_stress = common + N * 6 * 8 + E * 30 * 8, common + N * 6 * 8 + E * slots * 8, common + E * 14 * 8
    b_gather = E * (30 * 8 + 10 * 4) + N * (3 * 8 + 4)
    frac = lambda b, ms: b / (ms * 1e-3) / HBM  # noqa: E731
    print(f"config={cfg} elements={E} nodes={N} material={w['material']['kind']} solve: newton={st['newton']} "
          f"||g||={st['norm_g']:.3e}", flush=True)
    print(f"config={cfg} shape_point_ms={shape[0]:.4f} shape_gather_ms={shape[1]:.4f} shape_pair_ms={shape.sum():.4f} "
          f"sens_point_ms={sens[0]:.4f} stress_point_ms={stress[0]:.4f} "
          f"ratio_shape_point_to_stress_point={shape[0] / stress[0]:.2f} "
          f"bytes_MB shape/gather/sens/stress={b_shape / 1e6:.1f}/{b_gather / 1e6:.1f}/{b_sens / 1e6:.1f}/{b_stress / 1e6:.1f} "
          f"hbm_fraction shape/gather/sens/stress={frac(b_shape, shape[0]):.3f}/{frac(b_gather, shape[1]):.3f}/"
          f"{frac(b_sens, sens[0]):.3f}/{frac(b_stress, stress[0]):.3f} (medians of {4 * samples} x {reps} launches)", flush=True)
    print(f"config={cfg} adjoint_step_ms={adj['without'][0]:.3f} (cg iterations {adj['without'][1]}) "
          f"adjoint_step_with_X_bar_ms={adj['with'][0]:.3f} (cg iterations {adj['with'][1]}, rel_res {adj['with'][2]:.2e}) "
          f"difference_ms={adj['with'][0] - adj['without'][0]:.3f} (medians of {samples} host-clock samples)", flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="B,C")
    a = ap.parse_args()
    if tl.device_count() < 1:
        raise SystemExit("shape_timing.py needs a GPU")
    for cfg in a.configs.split(","):
        run(cfg, a.samples, a.reps)
