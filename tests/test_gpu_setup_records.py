"""Solve set-up from the element records (DESIGN 3g', TLFEA_SETUP_RECORDS): where the CG's product, the fine smoother and the
lambda_max product all run from the element records, the Newton loop leaves H unassembled.  It assembles the image rows of R
-- row I = sum over the children of w H[child, :], the row of the vertex's linear hat function -- and the fine block diagonal
instead, and the p-multigrid set-up sums Hc, D_c, sc_c and R from the image (form 4 of RetrievePmgLevelBuilt).  Everything
that still reads H gets it assembled on demand from the point records, or an error once they have moved.

Every configuration runs tests/setup_records_worker.py once in a fresh child (the switches are read once per process) with
TLFEA_SPMV_MATFREE=1 and TLFEA_PMG_FINE_MATFREE=1, which make the small meshes eligible; a dead or hung child ends the
session, as in tests/test_gpu_galerkin_rows.py.  `on` has TLFEA_SETUP_RECORDS=1, `off` has 0 and is the reference: the same
script, the same start state, the CSR set-up.

Meshes: the three of tests/galerkin_np.py (beam_3x2x1: 36 elements, less than one tile of 64, so the packed records have padding
lanes; box: 270 elements, interior vertices of 24 corner instances -- rows that span passes of 16; permuted: res4 in a random
order, R rows of 14..280 blocks, some on the global-memory image), a single element, two elements sharing a face, and the box
with only mid-edge nodes pinned (their parents free: the penalty reaches the image through the children's list alone).

Bounds, none fitted: fp64 operators (image rows, Hc, D) within 1e-12 of the largest entry, the bound of
tests/test_gpu_galerkin_rows.py; R as stored within one unit in the last place of float32 per entry (the fp64 values differ
near 1e-15 relative, far below half a float ulp, so almost every entry is equal: the share that differs is printed);
sc_c array_equal to 1/sqrt of the diagonal of the as-built Hc; CG counts equal; solutions within 1e-10 of the largest entry
(the suite's parity bar); true residuals against the CSR H at most the rel_tol of 1e-12 the solves are asked to reach."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import galerkin_rows_np as grn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {"TLFEA_SPMV_MATFREE": "1", "TLFEA_PMG_FINE_MATFREE": "1"}
ON, OFF = dict(BASE, TLFEA_SETUP_RECORDS="1"), dict(BASE, TLFEA_SETUP_RECORDS="0")
MESHES = ["beam_3x2x1", "box", "permuted", "one_tet", "two_tets", "mid_pins"]
STALE = "the point records are no longer those of that assembly"
_cache = {}


def run(cfg, env, tmp_path_factory):
    key = (json.dumps(cfg, sort_keys=True), json.dumps(env, sort_keys=True))
    if key in _cache:
        return _cache[key]
    tag = "_".join([cfg["mesh"], cfg.get("variant", "none"), "rec" + env.get("TLFEA_SETUP_RECORDS", "unset")])
    npz = str(tmp_path_factory.mktemp("setup_records") / (tag + ".npz"))
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
    try:
        r = subprocess.run([sys.executable, "-m", "tests.setup_records_worker", json.dumps(cfg), npz], cwd=ROOT,
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


def pair(mesh, tmp_path_factory):
    return run(dict(mesh=mesh), ON, tmp_path_factory), run(dict(mesh=mesh), OFF, tmp_path_factory)


def rel_max(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("mesh", MESHES)
def test_the_form_is_taken_and_h_is_assembled_only_on_demand(mesh, tmp_path_factory):
    (on, _), (off, _) = pair(mesh, tmp_path_factory)
    print(mesh, json.dumps(on["A"]), json.dumps(on["A_after_readback"]))
    for v in on["A"]:                                                    # three Newton iterations: no assembly of H
        assert v["form"] == dict(records=1, h_assemblies=0, h_current=False), v
        assert v["smoother"] == 1 and v["spmv"] == 1 and v["lin"], v
    assert on["A_after_readback"] == dict(records=1, h_assemblies=1, h_current=True), on   # the read-back assembles, once
    assert on["A_fourth"]["h_assemblies"] == 1 and not on["A_fourth"]["h_current"], on
    for k, v in enumerate(off["A"]):                                     # the switch at 0: every iteration assembles
        assert v["form"] == dict(records=0, h_assemblies=k + 1, h_current=True), v
    assert off["stale"] is None


@pytest.mark.parametrize("mesh", MESHES)
def test_stale_records_are_refused_with_the_stated_message(mesh, tmp_path_factory):
    (on, _), _ = pair(mesh, tmp_path_factory)
    assert on["stale"] is not None and STALE in on["stale"], on["stale"]


@pytest.mark.parametrize("mesh", MESHES)
def test_image_rows_are_the_children_s_weighted_rows_of_h(mesh, tmp_path_factory):
    (on, d_on), (_, d_off) = pair(mesh, tmp_path_factory)
    print(f"{mesh}: image rows vs sum_children w H[child, :] {on['image_relerr']:.3e} x max ({on['image_max']:.3e})")
    assert on["image_relerr"] <= 1e-12
    # H assembled on demand after the FIRST Newton iteration from the same start: the same kernel on the same records
    assert on["B_before_readback"]["h_assemblies"] == 0 and on["B_after_readback"]["h_assemblies"] == 1, on
    assert np.array_equal(d_on["H_val"], d_off["H_val"])


@pytest.mark.parametrize("mesh", MESHES)
def test_hc_and_the_fine_block_diagonal_against_the_csr_set_up(mesh, tmp_path_factory):
    (on, d_on), (off, d_off) = pair(mesh, tmp_path_factory)
    assert [v["hc_form"] for v in on["B_solves"]] == [4, 4] and [v["hc_form"] for v in off["B_solves"]] == [3, 3], (on, off)
    e_hc, e_d = rel_max(d_on["hc0"], d_off["hc0"]), rel_max(d_on["D0"], d_off["D0"])
    asym = grn.off_diagonal_asymmetry(d_on["c_off"], d_on["c_cols"], d_on["hc0"])
    print(f"{mesh}: Hc {e_hc:.3e}, fine D {e_d:.3e} x the largest entry; off-diagonal asymmetry of Hc {asym:.1e}")
    assert np.all(np.isfinite(d_on["hc0"])) and e_hc <= 1e-12 and e_d <= 1e-12
    assert asym == 0.0                                                   # every off-diagonal block the exact transpose of its mirror
    # two set-ups on one solver (the two linear solves): bit-identical
    assert np.array_equal(d_on["hc0"], d_on["hc1"]) and np.array_equal(d_on["D0"], d_on["D1"])
    assert np.array_equal(d_on["r_vals0"], d_on["r_vals1"])


@pytest.mark.parametrize("mesh", MESHES)
def test_r_and_the_scaling_formed_in_the_wave(mesh, tmp_path_factory):
    (_, d_on), (_, d_off) = pair(mesh, tmp_path_factory)
    assert np.array_equal(d_on["r_off"], d_off["r_off"]) and np.array_equal(d_on["r_cols"], d_off["r_cols"])
    a, b = d_on["r_vals0"].astype(np.float32), d_off["r_vals0"].astype(np.float32)
    assert np.array_equal(a.astype(np.float64), d_on["r_vals0"])         # R is stored in float: nothing lost above
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    differ = a != b
    print(f"{mesh}: {differ.mean():.2%} of the entries of R differ from the CSR set-up's, by at most "
          f"{float((np.abs(a - b) / ulp).max()):.1f} ulp")
    assert np.all(np.abs(a - b) <= ulp)
    c_off, c_cols = d_on["c_off"], d_on["c_cols"]
    row = np.repeat(np.arange(len(c_off) - 1), np.diff(c_off))
    diag = grn.blocks(c_off, d_on["hc1"])[row == c_cols]
    dd = np.stack([diag[:, c, c] for c in range(3)], axis=1).reshape(-1)
    assert len(dd) == 3 * (len(c_off) - 1) and np.all(dd > 0.0)
    assert np.array_equal(d_on["sc_c"], 1.0 / np.sqrt(dd))


@pytest.mark.parametrize("mesh", MESHES)
def test_solves(mesh, tmp_path_factory):
    (on, d_on), (off, d_off) = pair(mesh, tmp_path_factory)
    print(mesh, json.dumps(on["B_solves"]))
    assert [v["its"] for v in on["A"]] == [v["its"] for v in off["A"]], (on["A"], off["A"])   # the Newton loop's solves
    assert on["B_its"] == off["B_its"]
    assert [v["its"] for v in on["B_solves"]] == [v["its"] for v in off["B_solves"]], (on["B_solves"], off["B_solves"])
    for v in on["B_solves"]:
        assert v["form"]["records"] == 1 and v["smoother"] == 1, v
        assert v["rel"] <= 1e-12 and v["true_res"] <= 1e-12, v
    for k in ("x0", "x1"):
        dist = rel_max(d_on[k], d_off[k])
        print(f"{mesh} {k}: max |x - x_csr| = {dist:.3e} x max |x|")
        assert np.all(np.isfinite(d_on[k])) and dist <= 1e-10


def test_a_small_mesh_with_nothing_set_keeps_the_csr_set_up(tmp_path_factory):
    out, _ = run(dict(mesh="box"), {}, tmp_path_factory)
    assert [v["form"]["records"] for v in out["A"]] == [0, 0, 0], out
    assert [v["form"]["h_assemblies"] for v in out["A"]] == [1, 2, 3], out
    # forcing the fine smoother alone does not bring the form with it either
    out, _ = run(dict(mesh="box"), BASE, tmp_path_factory)
    assert [v["smoother"] for v in out["A"]] == [1, 1, 1], out
    assert [v["form"]["records"] for v in out["A"]] == [0, 0, 0] and out["B_solves"][0]["hc_form"] == 3, out


@pytest.mark.parametrize("variant", ["obstacle", "lincons", "per_element"])
def test_ineligible_cases_keep_the_csr_set_up_and_solve(variant, tmp_path_factory):
    out, _ = run(dict(mesh="box", variant=variant), ON, tmp_path_factory)
    print(variant, json.dumps(out["A"]), json.dumps(out["B_solves"]))
    assert [v["form"]["records"] for v in out["A"]] == [0, 0, 0], out
    assert [v["form"]["h_assemblies"] for v in out["A"]] == [1, 2, 3], out
    assert all(v["lin"] for v in out["A"]) and out["stale"] is None, out
    for v in out["B_solves"]:
        assert v["form"]["records"] == 0 and v["rel"] <= 1e-12 and v["true_res"] <= 1e-12, v
