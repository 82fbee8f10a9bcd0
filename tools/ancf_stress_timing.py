"""Cost of the ANCF stress recovery (DESIGN 3f') at config D (256 000 ANCF-3443 shells) and at config A's beam size next
to the residual launch of the Newton solver on the same mesh, in one process: medians and the min..max spread of
`samples` samples after warm-up, each sample the mean of `reps` back-to-back launches between one hipEvent pair
(tlfea_newton_time_kernels slot 0 for residual_kernel<16,48> / <8,12>, tlfea_ancf_time_stress_kernels for the point kernel,
the mesh-node gather and the totals), with and without point stresses, and each launch's share of the measured HBM copy
rate against the bytes it has to move.

    python tools/ancf_stress_timing.py [--samples 20] [--reps 10] [--configs D,A] | tee profiles/r09_ancf_stress_timing.txt"""
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


def algorithmic_bytes(E, S, Q, n_coef, nnz, points):
    """Bytes each launch has to move once: connectivity, coefficients and velocities, 3 S gradients and det J per point,
    the outputs; the gather's element records and node rows; the totals' element integrals and mass rows."""
    point = E * (S * 4 + Q * (3 * S + 1) * 8 + 10 * 8 + 4 * 8 + (Q * 6 * 8 if points else 0)) + n_coef * 3 * 8 * 2
    nodal = E * (S // 4) * (4 + 80) + (n_coef // 4) * (8 + 56)
    totals = E * 4 * 8 + nnz * 12 + n_coef * (8 + 48)
    return point, nodal, totals


def run(cfg, samples, reps):
    w = wl.build(cfg)
    d, s = wl.make_engine(tl, w)
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 300, 25, on_unconverged=1))
    x0 = w["x0"]
    d.UpdatePositions(x0[:, 0], x0[:, 1], x0[:, 2])
    s.BeginStep()
    s.NewtonIteration()  # warm-up: leaves a velocity and the solver's buffers
    E, n_coef = w["conn"].shape[0], len(w["x12"])
    off, _, _ = d.RetrieveMassCSRToCPU()
    nnz = int(off[-1])
    s.TimeKernels(reps)
    r = np.array([s.TimeKernels(reps)["residual"] for _ in range(samples)])
    res = np.median(r)
    print(f"config={cfg} kind={w['kind']} elements={E} coefficients={n_coef} residual_launch_ms={res:.4f} "
          f"[{r.min():.4f}..{r.max():.4f}] (median [min..max] of {samples} x {reps} launches)", flush=True)
    for points in (False, True):
        d.TimeANCFStressKernels(s, points, reps)
        a = np.array([d.TimeANCFStressKernels(s, points, reps) for _ in range(samples)])
        t = np.median(a, axis=0)
        b = algorithmic_bytes(E, d.S, d.Q, n_coef, nnz, points)
        frac = [bb / (tt * 1e-3) / HBM for bb, tt in zip(b, t)]
        print(f"config={cfg} point_stresses={int(points)} point_kernel_ms={t[0]:.4f} [{a[:, 0].min():.4f}..{a[:, 0].max():.4f}] "
              f"({t[0] / res:.2f}x residual) node_gather_ms={t[1]:.4f} [{a[:, 1].min():.4f}..{a[:, 1].max():.4f}] "
              f"totals_ms={t[2]:.4f} [{a[:, 2].min():.4f}..{a[:, 2].max():.4f}] "
              f"bytes_MB={b[0] / 1e6:.1f}/{b[1] / 1e6:.1f}/{b[2] / 1e6:.1f} hbm_fraction={frac[0]:.3f}/{frac[1]:.3f}/{frac[2]:.3f}",
              flush=True)
    d.CalcElementStress(s, want_points=True)
    en = d.GetANCFEnergies()
    print(f"config={cfg} energies strain={en.strain:.6e} kinetic={en.kinetic:.6e} volume={en.reference_volume:.6f} "
          f"max_nodal_von_mises={d.RetrieveANCFNodalStressToCPU().von_mises.max():.6e}", flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="D,A")
    a = ap.parse_args()
    if tl.device_count() < 1:
        raise SystemExit("ancf_stress_timing.py needs a GPU")
    for cfg in a.configs.split(","):
        run(cfg, a.samples, a.reps)
