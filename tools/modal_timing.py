"""Cost of the modal solve at configs B and C, informational: per config

  * milliseconds per block product Y = H X (spmm_block_kernel) at m = 8, 16, 32 columns -- hipEvents around 20 launches
    after a warm-up launch -- beside m x the fp64 SpMV of the CG iteration as TimeKernels reports it, and the bytes the
    product must move at least (H once, X read and Y written once) over the measured copy rate;
  * milliseconds per LOBPCG iteration: host clock around one ModalAnalysis call (it ends in a device synchronise) over
    its iteration count, after one untimed call; the call includes the assembly at the shifted time step, the
    preconditioner set-up and the re-assembly, so the figure is an upper bound of the iteration itself;
  * iterations to tol.

The mesh is the workload's, clamped as there, at rest, damping cleared (the modal call refuses a damped material).
No threshold hangs on any of it.

    python tools/modal_timing.py [--configs B,C] [--modes 6] [--tol 1e-8] | tee profiles/modal_timing.txt"""
import argparse
import ctypes
import importlib
import os
import sys
import time

HBM = 6.29e12  # bytes/s: the measured float4-copy rate of one MI355X

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="B,C")
    ap.add_argument("--modes", type=int, default=6)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    tl = importlib.import_module("total-lagrangian-fea_amd")
    wl = importlib.import_module("total-lagrangian-fea_amd.workloads")
    if tl.device_count() < 1:
        raise SystemExit("modal_timing.py needs a GPU")
    for cfg in a.configs.split(","):
        w = wl.build(cfg)
        d, _ = wl.make_engine(tl, w, with_solver=False)
        d.SetDamping(0.0, 0.0)
        s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
        s.Setup()
        s.SetParameters(tl.SyncedNewtonParams(*w["params"]))
        s.AnalyzeHessianSparsity()
        s.AssembleHessian()
        N = d.get_n_coef()
        nnz = ctypes.c_int()
        s._lib.tlfea_newton_hessian_nnz(s._h, ctypes.byref(nnz))
        nnz_blocks = nnz.value // 9
        spmv = s.TimeKernels(a.reps)["spmv"]
        print(f"config={cfg} nodes={N} blocks={nnz_blocks} fp64_spmv_ms={spmv:.4f}", flush=True)
        for m in (8, 16, 32):
            ms = s.ModalTimeSpmm(m, a.reps)
            least = 72.0 * nnz_blocks + 4.0 * nnz_blocks + 2 * 24.0 * N * m
            print(f"  spmm_block m={m}: {ms:.4f} ms, {m} x spmv = {m * spmv:.4f} ms ({m * spmv / ms:.2f}x), least bytes "
                  f"{least / 1e6:.1f} MB = {least / (ms * 1e-3) / HBM:.3f} of the copy rate", flush=True)
        for timed in (False, True):
            t0 = time.perf_counter()
            try:
                r = s.ModalAnalysis(a.modes, tol=a.tol, max_iter=a.max_iter)
            except tl.TlfeaError as e:
                r = e.partial
                print(f"  not converged: {e}", flush=True)
            dt = time.perf_counter() - t0
            if timed:
                print(f"  ModalAnalysis n_modes={a.modes} block={r.block} precond={r.precond}: {r.iterations} iterations to tol "
                      f"{a.tol:g} ({r.converged} converged), {1e3 * dt:.1f} ms per call, {1e3 * dt / max(r.iterations, 1):.2f} ms "
                      f"per iteration (call / iterations); f_hz = {r.freq_hz}", flush=True)
        del s
        d.Destroy()
