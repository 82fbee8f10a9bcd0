"""bench.py on one GPU: a plain run prints the headline line and nothing that needs runs of its own, --full adds the
per-kernel / per-stage figures, --dump-outputs writes what the last timed step computed, the same from run to run."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("element_stage", "stage_ms_per_step", "roofline", "roofline_all", "cpu_baseline")


def bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "S", *extra],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_plain_run_and_its_outputs(tmp_path):
    runs = [bench("--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / k)) for k in "ab"]
    for out in runs:
        assert out["steps"] == 4 and out["ms_per_step"] > 0 and out["config"]["last_solve_converged"]
        assert out["value"] * out["ms_per_step"] * 1e-3 == pytest.approx(out["config"]["elements_per_gpu"], rel=1e-3)
        assert not [k for k in FULL_ONLY if k in out]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["norm_g.npy", "position.npy", "rows.npy", "velocity.npy"]
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    b = {n[:-4]: np.load(tmp_path / "b" / n) for n in names}
    for k in a:
        assert a[k].dtype == np.float64 and a[k].shape == b[k].shape, k
        assert np.max(np.abs(a[k] - b[k])) <= 1e-12 * np.max(np.abs(b[k])), k   # same inputs, same outputs
    n = runs[0]["config"]["nodes_per_gpu"]
    assert a["position"].shape == a["velocity"].shape == (n, 3) and np.array_equal(a["rows"], np.arange(n))

    # the arrays are those of the timed path: replay prewarm-free warm-up + timed steps in this process
    tl = importlib.import_module("total-lagrangian-fea_amd")
    wl = importlib.import_module("total-lagrangian-fea_amd.workloads")
    w = wl.build("S")
    d, s = wl.make_engine(tl, w)
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 50000, 25, 0, 0.0, 0, 0, 0, 0))
    d.UpdatePositions(w["x0"][:, 0], w["x0"][:, 1], w["x0"][:, 2])
    for i in range(5):
        if i % 3 == 0:
            s.BeginStep()
        ng, _ = s.NewtonIteration()
    x, v = np.stack(d.RetrievePositionToCPU(), axis=1), s.RetrieveVelocityToCPU().reshape(-1, 3)
    del s
    d.Destroy()
    disp = np.max(np.abs(x - w["x0"]))
    assert disp > 0 and np.max(np.abs(a["position"] - x)) <= 1e-10 * disp + 8 * np.finfo(np.float64).eps * np.max(np.abs(x))
    assert np.max(np.abs(a["velocity"] - v)) <= 1e-10 * np.max(np.abs(v))
    assert a["norm_g"][0] == pytest.approx(ng, rel=1e-8)


def test_bench_full_run():
    out = bench("--steps", "3", "--warmup", "1", "--prewarm-s", "0", "--full", "--no-cpu-baseline")
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["roofline"]["kernel"] in out["roofline_all"] and out["element_stage"]["ms_per_step"] > 0
    assert out["stage_ms_per_step"]["pcg"] > 0 and "cpu_baseline" not in out
