"""The CG preconditioner pinned as an operator: z = M^-1 r from the device (ApplyPreconditioner, the function a CG
iteration calls) against the fp64 restatement tests/precond_np.py with the same storage rounding, vector by vector, for
every kernel form the preconditioner takes ("Linear solve").  Each configuration runs tests/precond_worker.py in a child
process (the library reads its TLFEA_* switches once), one child at a time.

Bounds.  The restatement with float32 work vectors against the same restatement with float64 ones (identical matrix
rounding) is the fp32 arithmetic floor of a configuration's operator; it is computed here, on the CPU, from numpy alone,
as the largest such distance over the configuration's test vectors.  The device must stay within 8 x that floor (a
different summation order across 8 to 32 lanes, the float32 L^-1 of the node-block form) for the operator match and for
the symmetry defect, and never looser than 1e-3 (where a dropped block of a 30-block row would pass).  A floor above 1e-4
fails the configuration: its polynomial is to be shortened, not the bound widened.  Where the device streams H itself
(cheb_bits 64) every operand is fp64 and the bound is 1e-10: eps 1.1e-16 x 12 steps x ~60 products per row x the
recurrence's growth (<= 1e2) leaves ~1e-11.  The iteration counts of LinearSolve and of the numpy PCG with the restated
operator may differ by what the CPU shows between float32 and float64 work vectors on that case, plus 2."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import precond_np as pn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AUTO = [0, 0.0, 0, 0]
LONG_AND_SHORT = dict(blocks_max_gt=32, blocks_min_lt=16)   # a second round of a 16-lane row, masked lanes past a row's end
# name, problem, [cheb_degree, cheb_kappa, cheb_bits, precond], environment, preconditions the worker asserts
CONFIGS = [
    ("1_poly12_fp16", "res2", [12, 400.0, 16, 1], {}, dict(precond=1, degree=12, store=16, lanes_fine=16, **LONG_AND_SHORT)),
    ("1_poly12_fp32", "res2", [12, 400.0, 32, 1], {}, dict(precond=1, degree=12, store=32, lanes_fine=16, **LONG_AND_SHORT)),
    ("1_poly12_fp64", "res2", [12, 400.0, 64, 1], {}, dict(precond=1, degree=12, store=64, **LONG_AND_SHORT)),
    ("2_poly24_auto", "res2", [0, 0.0, 0, 1], {}, dict(precond=1, degree=24, store=16, lanes_fine=16)),
    ("3_pmg2_res2", "res2", AUTO, {}, dict(precond=2, levels=2, ks=4, lanes_fine=16, lanes_vertex=8)),
    ("3_pmg2_bunny", "bunny", AUTO, {}, dict(precond=2, levels=2, ks=4, lanes_vertex=8, vertex_blocks_max_gt=16)),
    ("4_pmg2_ks2", "res2", AUTO, {"TLFEA_PMG_KS": "2"}, dict(precond=2, levels=2, ks=2)),
    ("4_pmg2_ks1", "res2", AUTO, {"TLFEA_PMG_KS": "1"}, dict(precond=2, levels=2, ks=1)),
    ("5_pmg3_res4", "res4", AUTO, {"TLFEA_PMG_LEVELS": "3"}, dict(precond=2, levels=3, identity_rows=True)),
    ("5_pmg3_bunny", "bunny", AUTO, {"TLFEA_PMG_LEVELS": "3"}, dict(precond=2, levels=3, identity_rows=True)),
    ("6_two_rows_poly", "res2", [0, 0.0, 0, 1], {"TLFEA_C32_BW_N": "0"}, dict(precond=1, two_rows=True)),
    ("6_two_rows_pmg", "res2", AUTO, {"TLFEA_C32_BW_N": "0"}, dict(precond=2, levels=2, two_rows=True)),
    ("7_lanes8", "res2", [12, 400.0, 16, 1], {"TLFEA_C32_LANES": "8"}, dict(precond=1, lanes_fine=8, blocks_max_gt=48)),
    ("7_lanes32", "res2", [12, 400.0, 16, 1], {"TLFEA_C32_LANES": "32"}, dict(precond=1, lanes_fine=32, blocks_min_lt=32)),
    ("8_shell_block12", "shell3443", AUTO, {}, dict(precond=1, block=12, degree=16)),
    ("8_plate_block12", "plate3443", AUTO, {}, dict(precond=1, block=12, degree=16)),
    ("8_plate_block12_lanes32", "plate3443", AUTO, {"TLFEA_C32_LANES": "32"}, dict(precond=1, block=12, lanes_fine=32)),
    ("9_shell_block3", "shell3443", AUTO, {"TLFEA_ANCF_BLOCK12": "0"}, dict(precond=1, block=3, degree=16)),
    ("10_beam3243", "beam3243", AUTO, {}, dict(precond=1, degree=16)),
    ("11_pmg2_smoother4", "res2", AUTO, {"TLFEA_PMG_SMOOTHER": "4"}, dict(precond=2, levels=2, ks=4, smoother=4)),
]


def state_of(data, which):
    st = {k: int(v) for k, v in zip(data["layout_keys"], data["layout" + which])}
    st["coef"] = data["coef" + which]
    return st


@pytest.mark.parametrize("name,problem,opts,env,expect", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_preconditioner_is_the_restated_operator(name, problem, opts, env, expect, tmp_path):
    npz = str(tmp_path / "case.npz")
    cfg = dict(name=name, problem=problem, opts=opts, expect=expect)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k in ("TLFEA_LIB_PATH", "TLFEA_PRECOND_REPORT")}
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "precond_worker.py"), json.dumps(cfg), npz], cwd=ROOT,
                           env=dict(clean, **env), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % name, returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):  # killed by a signal: a GPU fault or an abort ends the session
        pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s" % (name, r.returncode, r.stderr[-3000:]),
                    returncode=3)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    data = dict(np.load(npz, allow_pickle=False))
    names = [str(v) for v in data["names"]]

    # the fp32 arithmetic floor of this operator, on the CPU
    st = state_of(data, "")
    op64, op32 = pn.operator_from(data, st, np.float64), pn.operator_from(data, st, np.float32)
    floors = {}
    for nm, r_ in zip(names, data["R"]):
        z64 = op64(r_)
        floors[nm] = float(np.linalg.norm(op32(r_) - z64) / np.linalg.norm(z64))
    floor = max(floors.values())
    bound = 1e-10 if out["store"] == 64 else min(8.0 * floor, 1e-3)
    # the CPU's own spread of CG iteration counts between float32 and float64 work vectors
    st_e = state_of(data, "_solve")
    H = pn.unpack_csr("H", data)
    it64 = pn.pcg(H, data["b"], pn.operator_from(data, st_e, np.float64), 1e-12)[1]
    it32 = pn.pcg(H, data["b"], pn.operator_from(data, st_e, np.float32), 1e-12)[1]
    gap = abs(it32 - it64) + 2

    err, sym = max(out["err"].values()), max(out["sym"])
    line = ("%-24s store %2d  floor %.2e  bound %.2e  err(a) %.2e [%s]  sym(b) %.2e  its gpu %d numpy %d (cpu f32 %d f64 %d)"
            % (name, out["store"], floor, bound, err, max(out["err"], key=out["err"].get), sym, out["its_gpu"], out["its_np"],
               it32, it64))
    print(line)
    print(json.dumps(dict(out, floors=floors, bound=bound, its_cpu32=it32, its_cpu64=it64)))
    report = os.environ.get("TLFEA_PRECOND_REPORT")
    if report:
        with open(report, "a") as f:
            f.write(line + "\n")

    assert out["finite"]
    assert floor <= 1e-4, (name, floor, "shorten the polynomial of this configuration")
    assert out["zero_exact"], "M^-1 0 is not exactly zero"                                                  # (a)
    assert all(e <= bound for e in out["err"].values()), (bound, out["err"])                                 # (a)
    assert sym <= bound, (bound, out["sym"])                                                                 # (b)
    assert all(v > 0.0 for v in out["xMx"].values()), out["xMx"]                                             # (c)
    assert out["bitwise_repeat"] and out["bitwise_block_vs_single"]                                          # (d)
    assert out["rel_gpu"] <= 1e-12 and out["rel_np"] <= 1e-12 and out["x_relerr"] <= 1e-8
    assert abs(out["its_gpu"] - out["its_np"]) <= gap, (out["its_gpu"], out["its_np"], it32, it64)           # (e)
