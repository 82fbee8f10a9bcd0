"""Cost of the ANCF adjoint step (DESIGN 3j') at config D (256 000 ANCF-3443 shells) and config A (30 ANCF-3243 beams), in
one process per config: ancf_sens_point_kernel and its sums against ancf_stress_point_kernel<..., false> on the same mesh
(the yardstick: the same gradient stream) as medians of `samples` hipEvent pairs around `reps` back-to-back launches; one
forward Newton iteration and the whole adjoint step (device form, per-material and per-element outputs) as medians of
host-clock samples around calls that end in a device synchronise; the CG iterations of each, and the bytes the element
kernels have to move against the measured HBM copy rate.  Config A's material is damped; the adjoint refuses damping, so
the tool clears it.

    python tools/ancf_adjoint_timing.py [--samples 20] [--reps 10] [--configs D,A] | tee profiles/ancf_adjoint_timing.txt"""
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


def run(cfg, samples, reps, step_samples):
    import torch
    w = wl.build(cfg)
    d, s = wl.make_engine(tl, w)
    d.SetDamping(0.0, 0.0)
    p = list(w["params"])
    p[4] = 1  # one outer iteration: the step the adjoint differentiates
    p[1] = max(p[1], 1e-6)
    s.SetParameters(tl.SyncedNewtonParams(*p))
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 50000, 25))
    x0 = w["x0"]
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    s.BeginStep()
    for _ in range(3):  # warm-up: buffers, the preconditioner, the captured CG graphs
        s.NewtonIteration()
    E, N, S, Q = w["conn"].shape[0], len(w["x12"]), d.S, d.Q
    fwd, fwd_it = [], []
    for _ in range(step_samples):
        t0 = time.perf_counter()
        _, it = s.NewtonIteration()
        fwd.append(1e3 * (time.perf_counter() - t0))
        fwd_it.append(it)
    # a whole step from the start state again: its Newton loop leaves through inner_rtol of the first ||g||
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    s.SetVelocity(np.zeros(3 * N), np.zeros(3 * N))
    s.Solve()
    st = s.GetStats()
    s.ANCFAdjointReady()
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(7)
    n, nc = 3 * N, s.n_constraints
    _, slots = d.ANCFMaterialSensitivityShape()
    ins = [torch.randn(n, dtype=torch.float64, generator=gen).to(dev), torch.randn(n, dtype=torch.float64, generator=gen).to(dev),
           (torch.randn(nc, dtype=torch.float64, generator=gen) / p[3]).to(dev), None]
    z = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)  # noqa: E731
    outs = [z(n), z(n), z(n), z(nc), z(nc), z(3), z(slots), z(E * (slots - 1))]
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    cin, cout = binding.AdjointInC(*[ptr(t) for t in ins]), binding.AdjointOutC(*[ptr(t) for t in outs])
    torch.cuda.synchronize()
    s.ANCFAdjointStepDevice(cin, cout)
    adj, adj_it = [], []
    for _ in range(step_samples):
        t0 = time.perf_counter()
        it, rel = s.ANCFAdjointStepDevice(cin, cout)
        adj.append(1e3 * (time.perf_counter() - t0))
        adj_it.append(it)
    d.TimeANCFSensitivityKernels(reps)
    sens = np.median([d.TimeANCFSensitivityKernels(reps) for _ in range(samples)], axis=0)
    d.TimeANCFStressKernels(None, False, reps)
    stress = np.median([d.TimeANCFStressKernels(None, False, reps) for _ in range(samples)], axis=0)
    # bytes each element kernel has to move once: connectivity, Q x 3 S gradients, det J, the coefficient vectors; the
    # sensitivity kernel adds w and stores P doubles, the stress kernel stores its 10-double record and 4 integrals
    common = E * (S * 4 + Q * 3 * S * 8 + Q * 8) + N * 3 * 8
    b_sens, b_stress = common + N * 3 * 8 + E * (slots - 1) * 8, common + E * 14 * 8
    print(f"config={cfg} elements={E} coefficients={N} kind={w['kind']} solve: newton={st['newton']} ||g||={st['norm_g']:.3e}",
          flush=True)
    print(f"config={cfg} ancf_sens_point_ms={sens[0]:.4f} sens_sums_ms={sens[1]:.4f} sens_pair_ms={sens.sum():.4f} "
          f"ancf_stress_point_ms={stress[0]:.4f} ratio_sens_point_to_stress_point={sens[0] / stress[0]:.2f} "
          f"bytes_MB={b_sens / 1e6:.1f}/{b_stress / 1e6:.1f} hbm_fraction={b_sens / (sens[0] * 1e-3) / HBM:.3f}/"
          f"{b_stress / (stress[0] * 1e-3) / HBM:.3f} (medians of {samples} x {reps} launches)", flush=True)
    print(f"config={cfg} forward_newton_iteration_ms={np.median(fwd):.3f} (cg iterations {sorted(set(fwd_it))}) "
          f"adjoint_step_ms={np.median(adj):.3f} (cg iterations {sorted(set(adj_it))}, rel_res {rel:.2e}) "
          f"ratio={np.median(adj) / np.median(fwd):.2f} (medians of {step_samples} host-clock samples)", flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-samples", type=int, default=5)
    ap.add_argument("--configs", default="D,A")
    a = ap.parse_args()
    if tl.device_count() < 1:
        raise SystemExit("ancf_adjoint_timing.py needs a GPU")
    for cfg in a.configs.split(","):
        run(cfg, a.samples, a.reps, a.step_samples)
