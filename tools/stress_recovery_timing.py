"""Cost of the recovered stress (DESIGN 3f'') at config C (972 000 T10, SVK) and config B next to the launches of the stress
recovery it builds on, in one process: medians of 20 samples after warm-up, each sample the mean of `reps` back-to-back
launches between one hipEvent pair (tlfea_t10_time_stress_kernels with point stresses for stress_point_kernel and
stress_nodal_kernel, tlfea_t10_time_recovery_kernels for the element records, the nodal gather from them, the nodal gather
straight from the point blocks, the principal launches with directions, the error indicator and its totals), and each
launch's share of the measured HBM copy rate against the bytes it has to move.

    python tools/stress_recovery_timing.py [--samples 20] [--reps 10] [--configs C,B] | tee profiles/stress_recovery_timing.txt"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
tl = importlib.import_module("total-lagrangian-fea_amd")
wl = importlib.import_module("total-lagrangian-fea_amd.workloads")

HBM = 6.29e12  # bytes/s: the measured float4-copy rate of one MI355X (8.0e12 is the datasheet figure)
NAMES = ("element_records", "nodal_gather", "nodal_gather_direct", "principal", "error_indicator", "totals")


def algorithmic_bytes(E, N, inc):
    """Bytes each launch has to move once (a gather counts what every incidence reads, not what the caches absorb)."""
    elem = E * (30 * 8 + 5 * 8 + 32 * 8)
    vertex, edge = 4 * E, 6 * E                                   # incidences of vertices and of mid-edge nodes
    nodal = inc * 4 + vertex * (48 + 8) + edge * (96 + 8) + N * (8 + 56)
    direct = inc * (4 + 240 + 8) + N * (8 + 56)
    principal = N * (56 + 32 + 72) + E * (48 + 32 + 72)
    error = E * (10 * 4 + 30 * 8 + 5 * 8 + 10 * 48 + 3 * 8)
    totals = E * 3 * 8
    return elem, nodal, direct, principal, error, totals


def run(cfg, samples, reps):
    w = wl.build(cfg)
    d, s = wl.make_engine_t10(tl, w)
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 50000, 25))
    x0 = w["x0"]
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    for _ in range(3):  # warm-up: one time step of three Newton iterations leaves a deformed state
        if _ == 0:
            s.BeginStep()
        s.NewtonIteration()
    E, N = w["conn"].shape[0], w["X"].shape[0]
    d.TimeStressKernels(s, True, reps)
    base = np.median([d.TimeStressKernels(s, True, reps) for _ in range(samples)], axis=0)
    print(f"config={cfg} elements={E} nodes={N} material={w['material']['kind']} stress_point_kernel_points_ms={base[0]:.4f} "
          f"stress_nodal_kernel_ms={base[1]:.4f} (medians of {samples} x {reps} launches)", flush=True)
    d.TimeRecoveryKernels(reps)
    t = np.median([d.TimeRecoveryKernels(reps) for _ in range(samples)], axis=0)
    b = algorithmic_bytes(E, N, 10 * E)
    for name, tt, bb in zip(NAMES, t, b):
        print(f"config={cfg} {name}_ms={tt:.4f} ({tt / base[0]:.2f}x point kernel, {tt / base[1]:.2f}x nodal kernel) "
              f"bytes_MB={bb / 1e6:.1f} hbm_fraction={bb / (tt * 1e-3) / HBM:.3f}", flush=True)
    est = d.GetErrorEstimate()
    print(f"config={cfg} eta_rel={est.eta_rel:.6e} clamped={est.clamped} "
          f"max_recovered_von_mises={d.RetrieveRecoveredStressToCPU().von_mises.max():.6e}", flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="C,B")
    a = ap.parse_args()
    if tl.device_count() < 1:
        raise SystemExit("stress_recovery_timing.py needs a GPU")
    for cfg in a.configs.split(","):
        run(cfg, a.samples, a.reps)
