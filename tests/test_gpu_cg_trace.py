"""The CG iteration pinned kernel by kernel, in every launch form: SyncedNewtonSolver.CGTrace runs the solver's
own loop for k iterations and copies every iterate out; tests/cg_np.py judges each iteration locally -- product, direction,
update, the three dot products with their raw slots, and the preconditioner's output -- from the device's own previous
iterates, against long-double restatements and bounds derived from the number format and the launchers' grids (none is
tuned to the device).  Each configuration runs tests/cg_trace_worker.py in a child process (the library reads its TLFEA_*
switches once), one child at a time; the worker fails when the hook reports another form than the configuration names.

k = 4 iterations (6 where a residual replacement must fall inside), a seeded normal right-hand side, the perturbed SVK
state of tests/precond_worker.py.  Meshes: res2 (corner rows of 10 blocks: 3 deg = 30 < 32 lanes), plate3443 (12 x 12
node blocks) and structured_t10_box(20, 20, 19), whose 65 559 node rows are the smallest box over the 65 536 of the
XCD-eighth sweep (grid 512; an eighth rounds to 8 224 rows at 32 lanes and 8 256 at 16, so the last eighth is short).

Row classes.  A product kernel with L lanes per row takes no second round on a row with 3 deg < L, a partial one for
L < 3 deg < 2 L and several passes above; the worker demands every class the mesh kind can have.  A node of a T10 mesh has
at least the 10 nodes of one element in its row (3 deg >= 30) and the ANCF plate's rows hold 100+ blocks, so at 16 lanes
the first class and on the plate the first two cannot exist.

z of the polynomial and p-multigrid forms is compared with the restated operator of tests/precond_np.py by the rule of
tests/test_gpu_precond_operator.py, unchanged: 8 x the CPU's own fp32-vs-fp64 floor on these residuals, never looser than
1e-3, 1e-10 where H itself is streamed; a floor above 1e-4 fails.  On the box the first three z only.

TLFEA_CG_TRACE_REPORT=<file> appends one line per configuration with the worst ratio of each measured error to its bound
(profiles/cg_trace_margins.txt)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cg_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AUTO, JACOBI = [0, 0.0, 0, 0], [1, 0.0, 0, 0]
BASE = dict(fused=1, lanes=32, nt=0, tiled=1, xcd=0, graphs=1, spmv32=0, matfree=0, replaced_mask=0)
ALL, NO_SHORT, LONG = [0, 1, 2], [1, 2], [2]
# name, problem, opts, environment, k, the form the hook must report (over BASE), row classes demanded
CONFIGS = [
    ("jacobi_fused", "res2", JACOBI, {}, 4, dict(update=0), ALL),
    ("jacobi_unfused", "res2", JACOBI, {"TLFEA_PCG_FUSED": "0"}, 4, dict(update=0, fused=0), ALL),
    ("jacobi_lanes16", "res2", JACOBI, {"TLFEA_SPMV_LANES": "16"}, 4, dict(update=0, lanes=16), NO_SHORT),
    ("jacobi_unfused_lanes16", "res2", JACOBI, {"TLFEA_PCG_FUSED": "0", "TLFEA_SPMV_LANES": "16"}, 4,
     dict(update=0, fused=0, lanes=16), NO_SHORT),
    ("jacobi_nt", "res2", JACOBI, {"TLFEA_SPMV_NT": "1"}, 4, dict(update=0, nt=1), ALL),
    ("jacobi_unfused_nt", "res2", JACOBI, {"TLFEA_SPMV_NT": "1", "TLFEA_PCG_FUSED": "0"}, 4, dict(update=0, fused=0, nt=1), ALL),
    ("jacobi_untiled", "res2", JACOBI, {"TLFEA_ROW_TILED": "0"}, 4, dict(update=0, tiled=0), ALL),
    ("jacobi_eager", "res2", JACOBI, {"TLFEA_GRAPH": "0"}, 4, dict(update=0, graphs=0), ALL),
    ("poly_fp16", "res2", [12, 400.0, 16, 1], {}, 4, dict(update=2, precond=1, bits=16), ALL),
    ("poly_fp64", "res2", [12, 400.0, 64, 1], {}, 4, dict(update=1, precond=1, bits=64), ALL),
    ("pmg_auto", "res2", AUTO, {}, 4, dict(update=2, precond=2), ALL),
    ("pmg_unfused", "res2", AUTO, {"TLFEA_PCG_FUSED": "0"}, 4, dict(update=2, precond=2, fused=0), ALL),
    ("pmg_matfree", "res2", AUTO, {"TLFEA_SPMV_MATFREE": "1"}, 4, dict(update=2, precond=2, fused=0, matfree=1), ALL),
    ("mixed_r4", "res2", AUTO, {"TLFEA_SPMV32": "4"}, 6, dict(update=2, precond=2, spmv32=1, replaced_mask=1 << 3), ALL),
    ("mixed_r4_unfused", "res2", AUTO, {"TLFEA_SPMV32": "4", "TLFEA_PCG_FUSED": "0"}, 6,
     dict(update=2, precond=2, spmv32=1, replaced_mask=1 << 3, fused=0), ALL),
    ("plate_block12", "plate3443", AUTO, {}, 4, dict(update=1, precond=1, block12=1), LONG),
    ("xcd_jacobi", "box", JACOBI, {}, 4, dict(update=0, xcd=1), ALL),
    ("xcd_unfused_lanes16", "box", JACOBI, {"TLFEA_PCG_FUSED": "0", "TLFEA_SPMV_LANES": "16"}, 4,
     dict(update=0, xcd=1, fused=0, lanes=16), NO_SHORT),
    ("xcd_off", "box", JACOBI, {"TLFEA_XCD_ROWS": "0"}, 4, dict(update=0, xcd=0, xcd_mode=0), ALL),
    ("xcd_pmg", "box", AUTO, {}, 4, dict(update=2, precond=2, xcd=1), ALL),
]
Z_RECORDS = {"xcd_pmg": 3}


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    return str(tmp_path_factory.mktemp("cg_traces"))


@pytest.mark.parametrize("name,problem,opts,env,k,form,classes", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_iteration_is_the_restated_step(name, problem, opts, env, k, form, classes, traces):
    npz = os.path.join(traces, name + ".npz")
    cfg = dict(name=name, problem=problem, opts=opts, k=k, expect=dict(BASE, **form), classes=classes, z_records=Z_RECORDS.get(name))
    clean = {k_: v for k_, v in os.environ.items()
             if not k_.startswith("TLFEA_") or k_ in ("TLFEA_LIB_PATH", "TLFEA_CG_TRACE_REPORT")}
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cg_trace_worker.py"), json.dumps(cfg), npz], cwd=ROOT,
                           env=dict(clean, **env), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % name, returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):  # killed by a signal: a GPU fault or an abort ends the session
        pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s" % (name, r.returncode, r.stderr[-3000:]),
                    returncode=3)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    ratios = out.get("ratios", {})
    f = out["form"]
    line = ("%-24s N %6d  %s lanes %2d%s%s%s grid %3d %s update %d  rows %s  worst error / bound: %s%s"
            % (name, out["N"], "fused  " if f["fused"] else "unfused", f["lanes"], " nt" if f["nt"] else "", "" if f["tiled"] else " untiled",
               " xcd" if f["xcd"] else "", f["grid"], "graphs" if f["graphs"] else "eager ", f["update"], out["row_classes"],
               "  ".join("%s %.3f" % (key, ratios[key]) for key in sorted(ratios)),
               "  z floor %.2e bound %.2e" % (out["floor"], out["z_bound"]) if "floor" in out else ""))
    print(line)
    print(json.dumps(out))
    report = os.environ.get("TLFEA_CG_TRACE_REPORT")
    if report:
        with open(report, "a") as fh:
            fh.write(line + "\n")
    assert "failed" not in out, out["failed"]
    assert max(ratios.values()) <= 1.0, ratios
    if "floor" in out:
        assert out["floor"] <= 1e-4, (name, out["floor"], "shorten the polynomial of this configuration")
    assert out["bitwise_repeat"], ("two runs of the configuration differ: array -> [first record, entries, first entry]", out["repeat_differs"])


def load(traces, name):
    path = os.path.join(traces, name + ".npz")
    assert os.path.exists(path), "%s left no trace (its own test did not pass)" % name
    return dict(np.load(path, allow_pickle=False))


def pq_agree(a, b, N, lanes=32):
    """the p.q sums of two sweeps of bit-equal p_0, q_0: each within the dot bound of the long-double dot"""
    prod = a["p"][1].astype(np.longdouble) * a["q"][1].astype(np.longdouble)
    L = cg_np.ceil_div(N, cg_np.spmv_grid(N) * (1024 // lanes)) + 1 + cg_np.TAIL
    return abs(float(a["sums"][1, 2]) - float(b["sums"][1, 2])) <= 2 * (L + 2) * cg_np.U * float(np.abs(prod).sum())


def test_the_product_does_not_depend_on_the_sweep(traces):
    """the per-row arithmetic depends on LANES and FUSED only, not on which workgroup owns the row"""
    base = load(traces, "jacobi_fused")
    for other in ("jacobi_nt", "jacobi_untiled"):
        t = load(traces, other)
        assert np.array_equal(base["q"][1], t["q"][1]), other
        assert pq_agree(base, t, base["q"].shape[1] // 3), other
    a, b = load(traces, "xcd_jacobi"), load(traces, "xcd_off")
    assert np.array_equal(a["q"][1], b["q"][1])
    assert pq_agree(a, b, a["q"].shape[1] // 3)


def test_graph_replay_equals_eager_launches(traces):
    a, b = load(traces, "jacobi_fused"), load(traces, "jacobi_eager")
    for key in ("x", "r", "z", "p", "q", "sums"):
        assert np.array_equal(a[key], b[key]), key
