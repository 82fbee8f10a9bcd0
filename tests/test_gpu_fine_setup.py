"""The set-up of the fine level where the V-cycle's smoother runs from the element records (DESIGN 3g'): the fine level's
low-precision copy is converted only where something reads it.

A set-up that can still choose the matrix-free smoother defers the conversion; the read-back of the copy, TimeKernels and
every pass that streams the copy convert on demand, and a solver that never leaves the form never allocates the copy.  Every
scenario runs tests/fine_setup_worker.py once in a fresh child (the switches are read once per process) with
TLFEA_PMG_FINE_MATFREE=1, TLFEA_SPMV_MATFREE=1 and TLFEA_PMG_LEVELS=3; a dead or hung child ends the session, as in
tests/test_gpu_fine_matfree.py.  All children run ONE script (solves from one right-hand side, the hooks between them, then
cheb_bits = 16 set explicitly), so two children differ only in what a test is about: the lambda_max estimate is warm-started
from solve to solve, and equal histories give equal bits.

Meshes (tests/setup_kernels_worker.py): beam_3x2x1 (rows shorter than one wavefront), box (regular), permuted (res4 with
irregular row lengths and child counts).  Nothing here is a tolerance: states and counts are integers, copies and solutions
are compared bit for bit; the one inequality is the 1e-12 every solve is asked to reach."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {"TLFEA_SPMV_MATFREE": "1", "TLFEA_PMG_LEVELS": "3"}
ON = dict(BASE, TLFEA_PMG_FINE_MATFREE="1")
OFF = dict(BASE, TLFEA_PMG_FINE_MATFREE="0")
MESHES = ["beam_3x2x1", "box", "permuted"]
_cache = {}


def run(cfg, env, tmp_path_factory):
    key = (json.dumps(cfg, sort_keys=True), json.dumps(env, sort_keys=True))
    if key in _cache:
        return _cache[key]
    tag = "_".join([cfg["mesh"]] + ["%s-%s" % (k, v) for k, v in sorted(cfg.items()) if k != "mesh"])
    npz = str(tmp_path_factory.mktemp("fine_setup") / (tag + ".npz"))
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
    try:
        r = subprocess.run([sys.executable, "-m", "tests.fine_setup_worker", json.dumps(cfg), npz], cwd=ROOT,
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


def by_tag(out):
    """the records of the script's operations: solves under their tag, the hooks under their name"""
    return {o.get("tag", o["op"]): o for o in out["ops"]}


def n_solves(ops, upto):
    """set-ups a solve runs (LinearSolve and CGTrace) among the first `upto` + 1 operations"""
    return sum(1 for o in ops[:upto + 1] if o["op"] in ("solve", "trace"))


@pytest.mark.parametrize("mesh", MESHES)
def test_matrix_free_form_converts_only_on_demand(mesh, tmp_path_factory):
    out, data = run(dict(mesh=mesh), ON, tmp_path_factory)
    off, d_off = run(dict(mesh=mesh), OFF, tmp_path_factory)
    bare, d_bare = run(dict(mesh=mesh, hooks=False), ON, tmp_path_factory)
    o = by_tag(out)
    print(mesh, json.dumps(out["ops"]))
    assert out["precond"] == 2, out
    for tag in ("a0", "a1", "a2", "a3", "e0", "e1"):
        assert o[tag]["finite"] and o[tag]["rel"] <= 1e-12 and o[tag]["true_res"] <= 1e-12, o[tag]
    # two solves in the form: nothing allocated, nothing converted
    for tag in ("a0", "a1"):
        assert o[tag]["state"] == [0, 0, 0] and o[tag]["smoother"] == 1, o[tag]
    # the read-back converts once, and returns what a set-up with the form switched off stored for the same H and state
    assert o["retrieve"]["state"] == [16, 1, 1], o["retrieve"]
    for k in ("f_off", "f_cols", "f_vals", "sc_f", "sc_c"):
        assert np.array_equal(data[k], d_off[k]), k
    assert np.any(data["f_vals"] != 0.0)
    # a later solve in the form: the copy is stale again and stays so, the count does not move, the graphs replay
    assert o["a2"]["state"] == [16, 0, 1] and o["a2"]["smoother"] == 1, o["a2"]
    assert o["a2"]["its"] == o["a1"]["its"], (o["a1"], o["a2"])
    assert o["trace"]["graphs"] == 1 and o["trace"]["matfree"] == 1 and o["trace"]["state"] == [16, 0, 1], o["trace"]
    # TimeKernels prices the stream of the copy: it converts, the solve after it is the solve before it
    assert o["time"]["cheb_step"] > 0.0 and o["time"]["cheb_step_cycle"] > 0.0, o["time"]
    assert o["time"]["state"] == [16, 1, 2], o["time"]
    assert o["a3"]["state"] == [16, 0, 2] and o["a3"]["smoother"] == 1 and o["a3"]["its"] == o["a2"]["its"], o["a3"]
    # the hooks leave no trace in the solves: a child without them computes the same bits, and never allocates the copy
    ob = by_tag(bare)
    for tag in ("a0", "a1", "a2", "a3", "e0", "e1"):
        assert ob[tag]["its"] == o[tag]["its"], (tag, ob[tag], o[tag])
        assert np.array_equal(d_bare["x_" + tag], data["x_" + tag]), tag
    assert all(ob[tag]["state"] == [0, 0, 0] for tag in ("a0", "a1", "a2", "a3")), bare["ops"]
    assert ob["trace"]["graphs"] == 1 and ob["trace"]["state"] == [0, 0, 0], ob["trace"]
    assert ob["e0"]["state"] == [16, 1, 1] and ob["e1"]["state"] == [16, 1, 2], bare["ops"]
    # one system, one right-hand side: the solutions before and after the read-back agree as two solves to 1e-12 do (the
    # bar of tests/test_gpu_fine_matfree.py between its two smoothers; bit for bit they differ, the estimate moved on)
    assert np.abs(data["x_a2"] - data["x_a1"]).max() <= 1e-8 * np.abs(data["x_a1"]).max()


@pytest.mark.parametrize("mesh", MESHES)
def test_explicit_bits_turn_the_form_off_and_convert_every_solve(mesh, tmp_path_factory):
    out, data = run(dict(mesh=mesh), ON, tmp_path_factory)
    fresh, d_fresh = run(dict(mesh=mesh, explicit=True), ON, tmp_path_factory)
    o, f = by_tag(out), by_tag(fresh)
    print(mesh, json.dumps([o["e0"], o["e1"], f["e0"], f["e1"]]))
    # the same solver, switched: one conversion per solve from here on, into the storage it already holds
    assert o["e0"]["smoother"] == 0 and o["e1"]["smoother"] == 0, (o["e0"], o["e1"])
    assert o["e0"]["state"] == [16, 1, o["a3"]["state"][2] + 1] and o["e1"]["state"] == [16, 1, o["a3"]["state"][2] + 2]
    # a solver that had these options from its first solve (and the same history of solves): the same counts and residuals
    for k, rec in enumerate(fresh["ops"]):
        assert rec["smoother"] == 0 and rec["state"] == [16, 1, n_solves(fresh["ops"], k)], (k, rec)
    for tag in ("e0", "e1"):
        assert o[tag]["its"] == f[tag]["its"] and o[tag]["true_res"] == f[tag]["true_res"], (tag, o[tag], f[tag])
        assert o[tag]["rel"] <= 1e-12 and o[tag]["true_res"] <= 1e-12, o[tag]


@pytest.mark.parametrize("mesh", MESHES)
def test_switched_off_converts_once_per_solve(mesh, tmp_path_factory):
    off, _ = run(dict(mesh=mesh), OFF, tmp_path_factory)
    print(mesh, json.dumps(off["ops"]))
    for k, rec in enumerate(off["ops"]):
        assert rec["smoother"] == 0, rec
        assert rec["state"] == [16, 1, n_solves(off["ops"], k)], (k, rec)
        if rec["op"] == "solve":
            assert rec["finite"] and rec["rel"] <= 1e-12 and rec["true_res"] <= 1e-12, rec


# ---- R from H: the streamed build against the gather ------------------------------------------------------------------------
# Rows of R on these meshes have 14..42 (beam), 14..65 (box) and 14..280 (permuted) blocks: the default capacity of 128
# leaves nine rows of the permuted mesh to the gather kernel, 16 keeps only the shortest rows on the streamed kernel and 4
# none at all (every row through the row list).
STREAMS = [("default", {}), ("max16", {"TLFEA_ROP_STREAM_MAX": "16"}), ("max4", {"TLFEA_ROP_STREAM_MAX": "4"})]


@pytest.mark.parametrize("cap,cap_env", STREAMS, ids=[c[0] for c in STREAMS])
@pytest.mark.parametrize("mesh", MESHES)
def test_streamed_build_of_r_has_the_gathers_bits(mesh, cap, cap_env, tmp_path_factory):
    cfg = dict(mesh=mesh, what="rop")
    g, d_g = run(cfg, dict(ON, TLFEA_ROP_BUILD="gather"), tmp_path_factory)
    st, d_s = run(cfg, dict(ON, TLFEA_ROP_BUILD="stream", **cap_env), tmp_path_factory)
    print(mesh, cap, json.dumps(st))
    for o in (g, st):
        assert o["smoother"] == 1 and o["info"]["active"] == 1, o       # R was built from H, by the kernel under test
        assert o["bitwise_rebuild"], o
        assert o["state"] == [0, 0, 0], o
        assert all(v["smoother"] == 1 and v["rel"] <= 1e-12 and v["true_res"] <= 1e-12 for v in o["solves"]), o
    assert np.array_equal(d_g["off"], d_s["off"]) and np.array_equal(d_g["cols"], d_s["cols"])
    assert np.all(np.isfinite(d_s["vals"])) and np.any(d_s["vals"] != 0.0)
    assert np.array_equal(d_g["vals"], d_s["vals"])
    assert [v["its"] for v in g["solves"]] == [v["its"] for v in st["solves"]]
    assert np.array_equal(d_g["x0"], d_s["x0"]) and np.array_equal(d_g["x1"], d_s["x1"])
