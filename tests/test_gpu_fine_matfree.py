"""The fine smoother of the p-multigrid cycle from the element records (DESIGN 3g', TLFEA_PMG_FINE_MATFREE): the
preconditioner as an operator against the restatement tests/fine_matfree_np.py, R built from H against S_c P^T H S_f, and
solves with the switch on and off.  Every scenario runs tests/fine_matfree_worker.py once in a fresh child (the switches
are read once per process); a dead or hung child ends the session, as in tests/test_gpu_precond_operator.py.

Bounds.  The restatement forms the fine pass as the device does (the element map in the work type with the device's
normalisation, tests/fine_matfree_np.py ElementLevel).  The fp32 floor of a configuration is that restatement with float32
work vectors against float64 ones, on the CPU; the device must stay within min(8 x floor, 1e-3) for the operator match and
the symmetry defect, and a floor above 1e-4 fails the configuration.  One pass, in each of its three coefficient forms
(Chebyshev pair, restart pair (0, 1/theta), last pass), is compared with the fp64 CSR evaluation of the same formula in
the infinity norm relative to that of the result: within 8 x the CPU floor of that pass and never looser than 1e-4 (the
fp16 stream it replaces is good to about 2e-4 per entry); the r.z slots sum to r.z to 1e-12; two runs are bit-identical.  R: every entry within 2^-23 x the sum of the magnitudes of its terms (one rounding to
float32 of an fp64 sum), the rule of tests/test_gpu_setup_kernels.py.  Iteration counts with the switch on and off may
differ by what the CPU shows between float32 and float64 work vectors, plus 2.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fine_matfree_np as fm
from tests import precond_np as pn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = {"TLFEA_PMG_FINE_MATFREE": "1"}
OFF = {"TLFEA_PMG_FINE_MATFREE": "0"}
_cache = {}


def run(cfg, env, tmp_path, tag):
    key = (json.dumps(cfg, sort_keys=True), json.dumps(env, sort_keys=True))
    if key in _cache:
        return _cache[key]
    npz = str(tmp_path / (tag + ".npz"))
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
    try:
        r = subprocess.run([sys.executable, "-m", "tests.fine_matfree_worker", json.dumps(cfg), npz], cwd=ROOT,
                           env=dict(clean, **env), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % tag, returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s" % (tag, r.returncode, r.stderr[-3000:]),
                    returncode=3)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    data = dict(np.load(npz, allow_pickle=False))
    _cache[key] = (out, data)
    return out, data


def state_of(data, which):
    st = {k: int(v) for k, v in zip(data["layout_keys"], data["layout" + which])}
    st["coef"] = data["coef" + which]
    return st


OPERATOR = [("beam_ks2", "beam_3x2x1", {"TLFEA_PMG_KS": "2"}, 2, 2), ("beam_ks4", "beam_3x2x1", {}, 4, 2),
            ("box_ks2", "box", {"TLFEA_PMG_KS": "2"}, 2, 2), ("box_ks4", "box", {}, 4, 2),
            ("permuted_ks2", "permuted", {"TLFEA_PMG_KS": "2"}, 2, 2), ("permuted_ks4", "permuted", {}, 4, 2),
            ("box_levels3", "box", {"TLFEA_PMG_LEVELS": "3", "TLFEA_PMG_KS": "2"}, 2, 3),
            ("permuted_levels3", "permuted", {"TLFEA_PMG_LEVELS": "3"}, 4, 3)]


@pytest.mark.parametrize("name,mesh,env,ks,levels", OPERATOR, ids=[c[0] for c in OPERATOR])
def test_cycle_is_the_restated_operator_and_r_comes_from_h(name, mesh, env, ks, levels, tmp_path):
    out, data = run(dict(what="operator", mesh=mesh), dict(ON, **env), tmp_path, name)
    assert out["fine_smoother"] == 1 and out["fine_smoother_solve"] == 1, out
    assert out["precond"] == 2 and out["ks"] == ks and out["levels"] == levels and out["rop_active"] == 1, out
    st = state_of(data, "")
    op64, op32 = fm.element_operator_from(data, st, np.float64), fm.element_operator_from(data, st, np.float32)
    floor = 0.0
    for r_ in data["R"]:
        z64 = op64(r_)
        floor = max(floor, float(np.linalg.norm(op32(r_) - z64) / np.linalg.norm(z64)))
    bound = min(8.0 * floor, 1e-3)
    st_e = state_of(data, "_solve")
    H = pn.unpack_csr("H", data)
    it64 = pn.pcg(H, data["b"], fm.element_operator_from(data, st_e, np.float64), 1e-12)[1]
    it32 = pn.pcg(H, data["b"], fm.element_operator_from(data, st_e, np.float32), 1e-12)[1]
    err, sym = max(out["err"].values()), max(out["sym"])
    print("%-18s floor %.2e bound %.2e err %.2e [%s] sym %.2e R excess %.2e rel %.2e its gpu %d numpy %d (cpu f32 %d f64 %d)"
          % (name, floor, bound, err, max(out["err"], key=out["err"].get), sym, out["r_worst_excess"], out["r_worst_rel"],
             out["its_gpu"], out["its_np"], it32, it64))
    assert out["finite_z"] and out["finite"]
    assert floor <= 1e-4, (name, floor)
    assert out["zero_exact"], "M^-1 0 is not exactly zero"
    assert all(e <= bound for e in out["err"].values()), (bound, out["err"])
    assert sym <= bound, (bound, out["sym"])
    assert all(v > 0.0 for v in out["xMx"].values()), out["xMx"]
    assert out["bitwise_repeat"]
    assert out["r_pattern_equal"] and out["r_bitwise_rebuild"]
    assert out["r_worst_excess"] <= 0.0, out["r_worst_excess"]
    assert out["rel_gpu"] <= 1e-12 and out["true_res"] <= 1e-12 and out["rel_np"] <= 1e-12 and out["x_relerr"] <= 1e-8
    assert abs(out["its_gpu"] - out["its_np"]) <= abs(it32 - it64) + 2, (out["its_gpu"], out["its_np"], it32, it64)


@pytest.mark.parametrize("mesh", ["beam_3x2x1", "box", "permuted"])
def test_one_pass_in_each_coefficient_form(mesh, tmp_path):
    out, data = run(dict(what="operator", mesh=mesh), ON, tmp_path, mesh + "_ks4")
    H = pn.unpack_csr("H", data)
    L32, L64 = fm.ElementLevel(H, data, np.float32), fm.ElementLevel(H, data, np.float64)
    d, z, res, r = data["pass_d"], data["pass_z"], data["pass_res"], data["pass_r"]

    def dist(a, b):
        return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
    for nm, (c1, c2, w, last) in zip(data["pass_names"], data["pass_coef"]):
        o = out["pass"][str(nm)]
        if last:
            a, b = fm.last_pass(L32, d, z, res, r, c1, c2, w), fm.last_pass(L64, *(v.astype(np.float64) for v in (d, z, res)), r, c1, c2, w)
            floors = dict(d=dist(a[0], b[0]), z=dist(a[1], b[1]))
        else:
            a, b = L32.step(d, z, res, c1, c2, w), L64.step(*(v.astype(np.float64) for v in (d, z, res)), c1, c2, w)
            floors = dict(d=dist(a[0], b[0]), z=dist(a[1], b[1]), res=dist(a[2], b[2]))
        print(mesh, nm, " ".join("%s: floor %.2e device %.2e" % (k, f, o[k]) for k, f in floors.items()),
              "slots %s" % o.get("slots_rel"))
        assert o["finite"] and o["bitwise"], (nm, o)
        for k, f in floors.items():
            assert 0.0 < f <= 1e-4, (nm, k, f)
            assert o[k] <= min(8.0 * f, 1e-4), (nm, k, o[k], f)
        if last:
            assert o["slots_rel"] <= 1e-12 and o["slots_used"] >= 1, o
            assert o["rz_ref_rel"] <= 1e-4, o


@pytest.mark.parametrize("mesh", ["box", "permuted"])
def test_solve_with_the_switch_on_and_off(mesh, tmp_path):
    on, d_on = run(dict(what="solve", mesh=mesh), ON, tmp_path, mesh + "_on")
    off, d_off = run(dict(what="solve", mesh=mesh), OFF, tmp_path, mesh + "_off")
    forced, _ = run(dict(what="solve", mesh=mesh), {"TLFEA_SPMV_MATFREE": "1"}, tmp_path, mesh + "_spmv")
    op_out, op_data = run(dict(what="operator", mesh=mesh), ON, tmp_path, mesh + "_ks4")
    st_e = state_of(op_data, "_solve")
    H = pn.unpack_csr("H", op_data)
    it64 = pn.pcg(H, op_data["b"], fm.element_operator_from(op_data, st_e, np.float64), 1e-12)[1]
    it32 = pn.pcg(H, op_data["b"], fm.element_operator_from(op_data, st_e, np.float32), 1e-12)[1]
    print(mesh, "iterations on %d off %d (cpu f32 %d f64 %d)" % (on["its_gpu"], off["its_gpu"], it32, it64))
    assert on["fine_smoother_solve"] == 1 and off["fine_smoother_solve"] == 0, (on, off)
    # forcing the CG's product on a mesh below the size threshold leaves the smoother on the low-precision copy
    assert forced["spmv_mode"] == 1 and forced["fine_smoother_solve"] == 0, forced
    for o in (on, off):
        assert o["finite"] and o["rel_gpu"] <= 1e-12 and o["true_res"] <= 1e-12, o
    assert np.abs(d_on["x"] - d_off["x"]).max() <= 1e-8 * np.abs(d_off["x"]).max()
    assert abs(on["its_gpu"] - off["its_gpu"]) <= abs(it32 - it64) + 2, (on["its_gpu"], off["its_gpu"], it32, it64)


@pytest.mark.parametrize("E,h", [(1e12, 1e-5), (1e3, 1e-1)], ids=["stiff", "soft"])
def test_range_of_units(E, h, tmp_path):
    out, _ = run(dict(what="solve", mesh="box", material=[E, h]), ON, tmp_path, "box_E%g" % E)
    assert out["fine_smoother_solve"] == 1, out
    assert out["finite"] and out["rel_gpu"] <= 1e-12 and out["true_res"] <= 1e-12, out


@pytest.mark.parametrize("variant", ["per_element", "obstacle"])
def test_not_eligible_keeps_the_low_precision_copy(variant, tmp_path):
    out, _ = run(dict(what="solve", mesh="box", variant=variant), ON, tmp_path, "box_" + variant)
    assert out["fine_smoother_solve"] == 0, out
    assert out["finite"] and out["rel_gpu"] <= 1e-12, out
