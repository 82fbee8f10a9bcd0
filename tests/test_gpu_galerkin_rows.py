"""The T10 vertex level's Galerkin operator Hc = P^T H P summed from the row image of R (DESIGN 3g'): ONE arithmetic in every
mode.  Where a matrix-free set-up streams H to build R, the same wavefront sums the row of Hc from the image and scales R with
the sc_c it forms from the diagonal block (form 3); everywhere else the same device code runs alone (form 2); rows beyond the
image's capacity take it with the image in global memory.  So Hc must not depend on any switch.

Every configuration runs tests/galerkin_rows_worker.py once in a fresh child (the switches are read once per process) with
TLFEA_SPMV_MATFREE=1 and TLFEA_PMG_LEVELS=3; a dead or hung child ends the session, as in tests/test_gpu_fine_setup.py.  The
base child has TLFEA_PMG_FINE_MATFREE=1 and the streamed build; the others change one switch each:

    mf0     TLFEA_PMG_FINE_MATFREE=0       the fp16 copy smooths, R from the copy, Hc alone
    gather  TLFEA_ROP_BUILD=gather         matrix-free, R from H over its contribution lists, Hc alone
    rop0    TLFEA_PMG_RESTRICT_OP=0        no R at all (the fine residual pass restricts), Hc alone
    max16   TLFEA_ROP_STREAM_MAX=16        fused; the rows beyond 16 blocks (most) on the global-memory image
    max4    TLFEA_ROP_STREAM_MAX=4         fused; every row on the global-memory image

Meshes (tests/galerkin_np.py): beam_3x2x1 (24 coarse rows: less than one launch's worth), box (regular), permuted (res4 in a
random element order: R rows of 14..280 blocks, nine beyond the default capacity of 128).

Nothing here is fitted: Hc, R, sc_c, CG counts are compared bit for bit; the accuracy bound is the 1e-12 x max |Hc| of
tests/test_gpu_setup_kernels.py, the residual bound the 1e-12 every solve is asked to reach.  Solutions are compared bit for
bit among the children that run the same cycle (base, gather, max16, max4).  mf0 and rop0 run another preconditioner BY
their switch (fp16 copy in the smoother; the residual pass instead of R), so their CG iterates differ in the last bits
whatever builds Hc -- tests/test_gpu_fine_setup.py says the same of its two smoothers.  For them the CG counts must still be
equal and the true residuals at most 1e-12; the distance of their solutions from the base's is printed (2e-14 x max |x| when
this was written) and not asserted: any bound on it would follow from the residual bound alone and test nothing of Hc,
which is pinned directly above."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import galerkin_rows_np as grn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {"TLFEA_SPMV_MATFREE": "1", "TLFEA_PMG_LEVELS": "3", "TLFEA_PMG_FINE_MATFREE": "1"}
OTHERS = {"mf0": dict(BASE, TLFEA_PMG_FINE_MATFREE="0"), "gather": dict(BASE, TLFEA_ROP_BUILD="gather"),
          "rop0": dict(BASE, TLFEA_PMG_RESTRICT_OP="0"), "max16": dict(BASE, TLFEA_ROP_STREAM_MAX="16"),
          "max4": dict(BASE, TLFEA_ROP_STREAM_MAX="4")}
FORM = {"mf0": 2, "gather": 2, "rop0": 2, "max16": 3, "max4": 3}        # the kernel each set-up must have taken
SAME_CYCLE = ("gather", "max16", "max4")
MESHES = ["beam_3x2x1", "box", "permuted"]
_cache = {}


def run(mesh, env, tmp_path_factory):
    key = (mesh, json.dumps(env, sort_keys=True))
    if key in _cache:
        return _cache[key]
    tag = "_".join([mesh] + ["%s-%s" % (k[6:], v) for k, v in sorted(env.items()) if k not in BASE or env[k] != BASE[k]])
    npz = str(tmp_path_factory.mktemp("galerkin_rows") / (tag + ".npz"))
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
    try:
        r = subprocess.run([sys.executable, "-m", "tests.galerkin_rows_worker", json.dumps(dict(mesh=mesh)), npz], cwd=ROOT,
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


def children(mesh, tmp_path_factory):
    base = run(mesh, BASE, tmp_path_factory)
    return base, {tag: run(mesh, env, tmp_path_factory) for tag, env in OTHERS.items()}


@pytest.mark.parametrize("mesh", MESHES)
def test_hc_as_built_does_not_depend_on_the_mode(mesh, tmp_path_factory):
    (b, d_b), others = children(mesh, tmp_path_factory)
    print(mesh, json.dumps({k: b[k] for k in ("form", "smoother", "info", "cycle", "bitwise_rebuild")}))
    assert b["precond"] == 2 and b["smoother"] == 1 and b["info"]["active"] == 1, b
    assert b["form"] == 3, b                                            # the fused kernel left this Hc
    assert b["bitwise_rebuild"], b                                      # two set-ups of one H
    assert np.all(np.isfinite(d_b["hc"])) and np.any(d_b["hc"] != 0.0)
    assert np.array_equal(d_b["hc"], d_b["hc_alone"])                   # the stand-alone read-back of the same solver
    for tag, (o, d_o) in others.items():
        assert o["precond"] == 2 and o["form"] == FORM[tag], (tag, o)
        assert o["bitwise_rebuild"], (tag, o)
        assert np.array_equal(d_o["c_off"], d_b["c_off"]) and np.array_equal(d_o["c_cols"], d_b["c_cols"]), tag
        assert np.array_equal(d_o["hc"], d_b["hc"]), tag
        assert np.array_equal(d_o["hc_alone"], d_b["hc"]), tag


@pytest.mark.parametrize("mesh", MESHES)
def test_hc_is_pt_h_p_and_its_lower_triangle_the_exact_transpose(mesh, tmp_path_factory):
    (b, _), others = children(mesh, tmp_path_factory)
    for tag, o in [("base", b)] + [(t, v[0]) for t, v in others.items()]:
        print(f"{mesh} {tag}: Hc vs P^T H P {o['hc_relerr']:.3e} x max |Hc| ({o['hc_max']:.3e}), off-diagonal asymmetry "
              f"{o['hc_asym_offdiag']:.1e}")
        assert o["hc_relerr"] <= 1e-12, (tag, o)
        assert o["hc_asym_offdiag"] == 0.0, (tag, o)


@pytest.mark.parametrize("mesh", MESHES)
def test_r_and_the_scaling_formed_in_the_wave(mesh, tmp_path_factory):
    (b, d_b), others = children(mesh, tmp_path_factory)
    g, d_g = others["gather"]
    assert g["smoother"] == 1 and g["info"]["active"] == 1, g           # R from H there too, scaled with the stored sc_c
    assert np.all(np.isfinite(d_b["r_vals"])) and np.any(d_b["r_vals"] != 0.0)
    for tag in ("gather", "max16", "max4"):
        d_o = others[tag][1]
        assert np.array_equal(d_o["r_off"], d_b["r_off"]) and np.array_equal(d_o["r_cols"], d_b["r_cols"]), tag
        assert np.array_equal(d_o["r_vals"], d_b["r_vals"]), tag
    # the stored scaling is 1/sqrt of the diagonal of the Hc the set-up left, in every child
    c_off, c_cols = d_b["c_off"], d_b["c_cols"]
    row = np.repeat(np.arange(len(c_off) - 1), np.diff(c_off))
    diag = grn.blocks(c_off, d_b["hc"])[row == c_cols]
    dd = np.stack([diag[:, c, c] for c in range(3)], axis=1).reshape(-1)
    assert len(dd) == 3 * (len(c_off) - 1) and np.all(dd > 0.0)
    want = 1.0 / np.sqrt(dd)
    assert np.array_equal(d_b["sc_c"], want)
    for tag, (_, d_o) in others.items():
        assert np.array_equal(d_o["sc_c"], want), tag


@pytest.mark.parametrize("mesh", MESHES)
def test_solves_do_not_depend_on_how_hc_was_built(mesh, tmp_path_factory):
    (b, d_b), others = children(mesh, tmp_path_factory)
    print(mesh, json.dumps(b["solves"]))
    for tag, o in [("base", b)] + [(t, v[0]) for t, v in others.items()]:
        for v in o["solves"]:
            assert v["finite"] and v["rel"] <= 1e-12 and v["true_res"] <= 1e-12, (tag, v)
    its = [v["its"] for v in b["solves"]]
    for tag, (o, d_o) in others.items():
        assert [v["its"] for v in o["solves"]] == its, (tag, o["solves"], b["solves"])
        for k in ("x0", "x1"):
            if tag in SAME_CYCLE:
                assert all(v["smoother"] == 1 for v in o["solves"]), (tag, o)
                assert np.array_equal(d_o[k], d_b[k]), (tag, k)
            else:                                                       # another preconditioner by the switch itself (docstring)
                assert all(v["smoother"] == 0 for v in o["solves"]), (tag, o)
                diff = float(np.abs(d_o[k] - d_b[k]).max() / np.abs(d_b[k]).max())
                print(f"{mesh} {tag} {k}: max |x - x_base| = {diff:.3e} x max |x| (printed, not asserted)")
