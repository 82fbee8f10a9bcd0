"""The V-cycle's restriction through the stored operator R = S_c P^T S_f^-1 Hs ("Linear solve") on the device.
Each case runs tests/restrict_op_worker.py in a child process (the library reads its TLFEA_* switches once), one child at
a time; a child is run once and shared by the tests that read it.

  * R against its definition, recomputed in fp64 from the fine copy AS STORED and both scalings (retrieved from the
    device): identical pattern, every entry within 2^-23 x the sum of |terms| (one fp32 rounding of an fp64 sum, with a
    factor 2 of margin), two builds bit-identical.  res2 and bunny, storage 16 and 32 bits.
  * The operator on the new path for ks = 1, 2, 4, two and three levels, with the bound of
    tests/test_gpu_precond_operator.py: min(8 x the fp32 floor of the restated cycle, 1e-3) for the match with the fp64
    restatement and for the symmetry defect; M^-1 0 = 0; repeats and block application bit-identical.
  * The fallback (TLFEA_PMG_RESTRICT_OP=0) on the same vectors: the same bound; both paths solve to 1e-12 on the true
    residual; their iteration counts differ by no more than the CPU's own float32 / float64 gap plus 2.
  * One Newton step with and without TLFEA_GRAPH=0: identical iteration counts, bit-identical velocities.

Shapes: beam_3x2x1 (rows of R shorter than one round of lanes), res2 (fine rows of 10..57 blocks, rows of R that need a
second round), bunny (unstructured, no pinned nodes)."""
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
_RUNS = {}


def run_worker(mode, cfg, env, tmp_path_factory):
    key = (mode, json.dumps(cfg, sort_keys=True), json.dumps(env, sort_keys=True))
    if key in _RUNS:
        return _RUNS[key]
    npz = str(tmp_path_factory.mktemp("rop") / "case.npz")
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "restrict_op_worker.py"), mode, json.dumps(cfg), npz],
                           cwd=ROOT, env=dict(clean, **env), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % cfg["name"], returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):  # killed by a signal: a GPU fault or an abort ends the session
        pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s"
                    % (cfg["name"], r.returncode, r.stderr[-3000:]), returncode=3)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [json.loads(v) for v in r.stdout.strip().splitlines() if v.startswith("{")]
    _RUNS[key] = (lines, npz)
    return _RUNS[key]


# ---- R against its definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("problem", ["res2", "bunny"])
def test_r_is_its_definition(problem, bits, tmp_path_factory):
    cfg = dict(name="build_%s_%d" % (problem, bits), problem=problem, opts=[0, 0.0, bits, 0])
    (out,), _ = run_worker("build", cfg, {}, tmp_path_factory)
    print(json.dumps(out))
    assert out["info"]["fine_bits"] == bits
    assert out["copy_is_stored_type"] and out["r_is_float32"]
    assert out["pattern_equal"]
    assert out["worst_excess"] <= 0.0, out
    assert out["bitwise_rebuild"]
    if problem == "res2":   # what this shape is here for: short and long fine rows, rows of R beyond one round of lanes
        avg = out["info"]["blocks"] / out["info"]["n_coarse"]
        lanes = 32 if avg > 36.0 else (16 if avg > 18.0 else 8)     # the launcher's rule
        assert out["fine_rows_min"] <= 10 and out["fine_rows_max"] >= 57 and out["rows_max"] > 2 * lanes, out


# ---- the operator --------------------------------------------------------------------------------------------------------
def state_of(data, which):
    st = {k: int(v) for k, v in zip(data["layout_keys"], data["layout" + which])}
    st["coef"] = data["coef" + which]
    return st


def operator_case(problem, levels, ks, bits, rop, tmp_path_factory):
    """one child of the operator comparison + the CPU's floor and iteration gap for it (shared between tests)"""
    name = "%s_l%d_ks%d_b%d_rop%d" % (problem, levels, ks, bits, rop)
    key = ("case", name)
    if key in _RUNS:
        return _RUNS[key]
    env = {"TLFEA_PMG_KS": str(ks), "TLFEA_PMG_LEVELS": str(levels)}
    if not rop:
        env["TLFEA_PMG_RESTRICT_OP"] = "0"
    cfg = dict(name=name, problem=problem, opts=[0, 0.0, bits, 0], expect=dict(precond=2, levels=levels, ks=ks, smoother=1))
    (out, seen), npz = run_worker("operator", cfg, env, tmp_path_factory)
    data = dict(np.load(npz, allow_pickle=False))
    st = state_of(data, "")
    op64, op32 = pn.operator_from(data, st, np.float64), pn.operator_from(data, st, np.float32)
    floor = 0.0
    for r_ in data["R"]:
        z64 = op64(r_)
        floor = max(floor, float(np.linalg.norm(op32(r_) - z64) / np.linalg.norm(z64)))
    st_e = state_of(data, "_solve")
    H = pn.unpack_csr("H", data)
    it64 = pn.pcg(H, data["b"], pn.operator_from(data, st_e, np.float64), 1e-12)[1]
    it32 = pn.pcg(H, data["b"], pn.operator_from(data, st_e, np.float32), 1e-12)[1]
    res = dict(out=out, seen=seen, floor=floor, bound=min(8.0 * floor, 1e-3), gap=abs(it32 - it64) + 2, it32=it32, it64=it64)
    print("%-28s active %d  floor %.2e  bound %.2e  err %.2e  sym %.2e  its gpu %d numpy %d (cpu f32 %d f64 %d)  true rel %.2e  min x.Mx %.2e"
          % (name, seen["active"], floor, res["bound"], max(out["err"].values()), max(out["sym"]), out["its_gpu"],
             out["its_np"], it32, it64, seen["true_rel"], min(out["xMx"].values())))
    _RUNS[key] = res
    return res


def check_operator(c):
    out, bound = c["out"], c["bound"]
    assert out["finite"]
    assert c["floor"] <= 1e-4, c["floor"]
    assert out["zero_exact"], "M^-1 0 is not exactly zero"
    assert all(e <= bound for e in out["err"].values()), (bound, out["err"])
    assert max(out["sym"]) <= bound, (bound, out["sym"])
    # (x.Mx > 0 on the test vectors is a property of the cycle's parameters, not of the restriction: the one-term smoother
    # with three levels on bunny gives -0.006 on an impulse on both paths and in the restatement; it is printed, not asserted)
    assert out["bitwise_repeat"] and out["bitwise_block_vs_single"]
    assert out["rel_gpu"] <= 1e-12 and c["seen"]["true_rel"] <= 1e-12, (out["rel_gpu"], c["seen"]["true_rel"])
    assert abs(out["its_gpu"] - out["its_np"]) <= c["gap"], (out["its_gpu"], out["its_np"], c["it32"], c["it64"])


NEW_PATH = [("res2", 2, 1, 16), ("res2", 2, 2, 16), ("res2", 2, 4, 16), ("bunny", 3, 1, 16), ("bunny", 3, 2, 16),
            ("bunny", 3, 4, 16), ("beam_3x2x1", 2, 2, 16), ("res2", 2, 2, 32), ("res2", 3, 2, 16), ("bunny", 2, 2, 16)]


@pytest.mark.parametrize("problem,levels,ks,bits", NEW_PATH, ids=["%s_l%d_ks%d_b%d" % c for c in NEW_PATH])
def test_operator_on_the_new_path(problem, levels, ks, bits, tmp_path_factory):
    c = operator_case(problem, levels, ks, bits, True, tmp_path_factory)
    assert c["seen"]["active"] == 1, c["seen"]
    check_operator(c)


FALLBACK = [("res2", 2, 2, 16), ("bunny", 3, 2, 16)]


@pytest.mark.parametrize("problem,levels,ks,bits", FALLBACK, ids=["%s_l%d_ks%d_b%d" % c for c in FALLBACK])
def test_fallback_is_the_same_operator(problem, levels, ks, bits, tmp_path_factory):
    new = operator_case(problem, levels, ks, bits, True, tmp_path_factory)
    old = operator_case(problem, levels, ks, bits, False, tmp_path_factory)
    assert old["seen"]["active"] == 0 and new["seen"]["active"] == 1, (old["seen"], new["seen"])
    check_operator(old)
    assert abs(new["out"]["its_gpu"] - old["out"]["its_gpu"]) <= new["gap"], (new["out"]["its_gpu"], old["out"]["its_gpu"], new["gap"])


# ---- graph against eager ----------------------------------------------------------------------------------------------------
def test_graph_and_eager_newton_step_agree(tmp_path_factory):
    cfg = dict(name="newton_res2", problem="res2")
    (g,), npz_g = run_worker("newton", cfg, {}, tmp_path_factory)
    (e,), npz_e = run_worker("newton", cfg, {"TLFEA_GRAPH": "0"}, tmp_path_factory)
    print(json.dumps(dict(graph=g, eager=e)))
    assert g["active"] == 1 and e["active"] == 1 and g["precond"] == 2
    assert g["pcg_iters"] == e["pcg_iters"] and g["pcg_iters"] > 0
    assert np.array_equal(np.load(npz_g)["v"], np.load(npz_e)["v"])
