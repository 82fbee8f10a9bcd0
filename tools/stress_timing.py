"""Cost of the stress recovery at config C (972 000 T10, SVK) and config B next to the residual launch of
the Newton solver, in one process: medians of 20 samples after warm-up, each sample the mean of `reps` back-to-back
launches between one hipEvent pair (tlfea_newton_time_kernels for the residual, tlfea_t10_time_stress_kernels for the
point and element kernel, the nodal gather and the totals), with and without point stresses, and each launch's share of
the measured HBM copy rate against the bytes it has to move.

    python tools/stress_timing.py [--samples 20] [--reps 10] [--configs C,B] | tee profiles/r07_stress_timing.txt"""
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


def algorithmic_bytes(E, N, inc, nnz, points, with_v):
    """Bytes each launch has to move once: connectivity, positions, 150 gradients, det J and the outputs."""
    point = E * (10 * 4 + 150 * 8 + 5 * 8 + 10 * 8 + 4 * 8 + (30 * 8 if points else 0)) + N * 3 * 8 * (2 if with_v else 1)
    nodal = inc * (4 + 80) + N * (8 + 56)
    totals = E * 4 * 8 + (nnz * 12 + N * (8 + 48) if with_v else 0)
    return point, nodal, totals


def run(cfg, samples, reps):
    w = wl.build(cfg)
    d, s = wl.make_engine_t10(tl, w)
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 50000, 25))
    x0 = w["x0"]
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    for _ in range(3):  # warm-up: one time step of three Newton iterations leaves a velocity and the solver's buffers
        if _ == 0:
            s.BeginStep()
        s.NewtonIteration()
    E, N = w["conn"].shape[0], w["X"].shape[0]
    off, _, _ = d.RetrieveMassCSRToCPU()
    nnz = int(off[-1])
    s.TimeKernels(reps)
    res = np.median([s.TimeKernels(reps)["residual"] for _ in range(samples)])
    print(f"config={cfg} elements={E} nodes={N} material={w['material']['kind']} residual_launch_ms={res:.4f} "
          f"(median of {samples} x {reps} launches)", flush=True)
    for points in (False, True):
        d.TimeStressKernels(s, points, reps)
        t = np.median([d.TimeStressKernels(s, points, reps) for _ in range(samples)], axis=0)
        b = algorithmic_bytes(E, N, 10 * E, nnz, points, True)
        frac = [bb / (tt * 1e-3) / HBM for bb, tt in zip(b, t)]
        print(f"config={cfg} point_stresses={int(points)} point_element_ms={t[0]:.4f} ({t[0] / res:.2f}x residual) "
              f"nodal_gather_ms={t[1]:.4f} totals_ms={t[2]:.4f} bytes_MB={b[0] / 1e6:.1f}/{b[1] / 1e6:.1f}/{b[2] / 1e6:.1f} "
              f"hbm_fraction={frac[0]:.3f}/{frac[1]:.3f}/{frac[2]:.3f}", flush=True)
    d.CalcStress(s, points=True)
    en = d.GetEnergies()
    print(f"config={cfg} energies strain={en.strain:.6e} kinetic={en.kinetic:.6e} volume={en.reference_volume:.6f} "
          f"max_nodal_von_mises={d.RetrieveNodalStressToCPU().von_mises.max():.6e}", flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="C,B")
    a = ap.parse_args()
    if tl.device_count() < 1:
        raise SystemExit("stress_timing.py needs a GPU")
    for cfg in a.configs.split(","):
        run(cfg, a.samples, a.reps)
