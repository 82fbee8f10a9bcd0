"""The kernels a solve runs once, before its first CG iteration ("Linear solve"): the vertex-level Galerkin gather
over the upper triangle with its mirror store, the third-level Galerkin sum with 16 lanes per aggregate pair, the build of
R with its per-row table of child factors, and the fine lambda_max estimate through the matrix-free pair.

Meshes (tests/galerkin_np.py): beam_3x2x1, the structured 5 x 3 x 3 box, res4 in a permuted element order; the third level
is forced (TLFEA_PMG_LEVELS=3) and so is the matrix-free product (TLFEA_SPMV_MATFREE=1).  The switches are read once per
process: every (mesh, TLFEA_LMAX_MATFREE) pair runs once in a fresh child, shared by the tests below.

  * Hc against NumPy's P^T H P below 1e-12 x max |Hc| (the bound of tests/test_gpu_pmg3.py); every off-diagonal block the
    exact transpose of its mirror, Hc - Hc^T = 0 there.  A DIAGONAL block is summed in full, as before: inside it (d, e)
    and (e, d) are sums of the same numbers in two orders, so its own asymmetry is rounding and is held to the same 1e-12.
  * H3 against P2^T Hc P2 below 1e-12; Hc, H3 and R bit-identical over two builds.
  * the aggregate pairs' lists: one mesh has a pair with fewer than 16 contributions (a partial round of the lanes), one a
    pair with more (the loop).
  * R against its fp64 definition within 2^-23 x the sum of |terms| (tests/test_gpu_restrict_op.py).
  * cold fine lambda_max with TLFEA_LMAX_MATFREE=1 against =0 below 1e-12 relative: the products differ by ~6e-16 relative
    (profiles/r16_matfree_compact.txt section 8) over 17 normalised steps; the hook's flag says which product ran; the
    solves that follow take the same number of CG iterations and reach the same true residual to 1e-3 relative."""
import json
import os
import subprocess
import sys

import pytest

from tests import galerkin_np as gn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def run(what, mesh, lmax_matfree):
    key = (what, mesh, lmax_matfree)
    if key in _RUNS:
        return _RUNS[key]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
    env = dict(clean, TLFEA_PMG_LEVELS="3", TLFEA_SPMV_MATFREE="1", TLFEA_LMAX_MATFREE=lmax_matfree)
    try:
        r = subprocess.run([sys.executable, "-m", "tests.setup_kernels_worker", what, mesh], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % mesh, returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):  # killed by a signal: a GPU fault or an abort ends the session
        pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s"
                    % (mesh, r.returncode, r.stderr[-3000:]), returncode=3)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads([v for v in r.stdout.splitlines() if v.startswith("{")][-1])
    print(json.dumps(out))
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("mesh", gn.MESHES)
def test_vertex_galerkin(mesh):
    out = run("full", mesh, "1")
    assert out["assembly"] == 3 and out["precond"] == 2
    assert out["H_asym"] <= 1e-12, out                                  # what the mirror store rests on
    assert out["hc_relerr"] < 1e-12, out
    assert out["hc_asym_offdiag"] == 0.0, out
    assert out["hc_asym_diag_rel"] < 1e-12, out
    assert out["hc_bitwise_rebuild"], out


@pytest.mark.parametrize("mesh", gn.MESHES)
def test_level3_galerkin(mesh):
    out = run("full", mesh, "1")
    assert out["n_aggregates"] > 0 and out["cycle"]["levels"] == 3, out
    assert out["h3_relerr"] < 1e-12, out
    assert out["h3_bitwise_rebuild"], out


def test_level3_lists_cover_the_partial_round_and_the_loop():
    lo = min(run("full", m, "1")["pair_contributions"][0] for m in gn.MESHES)
    hi = max(run("full", m, "1")["pair_contributions"][1] for m in gn.MESHES)
    print("contributions per aggregate pair: %d ... %d" % (lo, hi))
    assert 1 <= lo < 16 < hi


@pytest.mark.parametrize("mesh", gn.MESHES)
def test_restricted_operator(mesh):
    out = run("full", mesh, "1")
    assert out["rop_info"]["active"] == 1, out
    assert out["r_pattern_equal"], out
    assert out["r_worst_excess"] <= 0.0, out
    assert out["r_bitwise_rebuild"], out
    # the preconditioner hook is a caller outside the solve: its estimate keeps the CSR product
    assert out["hook_lambda"][3] is False, out


@pytest.mark.parametrize("mesh", gn.MESHES)
def test_lambda_max_through_the_matrix_free_pair(mesh):
    new, old = run("full", mesh, "1"), run("solve", mesh, "0")
    cold_new, cold_old = new["solves"][0], old["solves"][0]
    assert cold_new["mode"] == 1 and cold_old["mode"] == 1              # both solves iterate with the matrix-free pair
    assert cold_new["lam"][3] is True and cold_old["lam"][3] is False
    rel = abs(cold_new["lam"][0] - cold_old["lam"][0]) / cold_old["lam"][0]
    print("%s: cold lambda_max %.15e (matrix-free) %.15e (CSR), relative difference %.3e"
          % (mesh, cold_new["lam"][0], cold_old["lam"][0], rel))
    assert cold_old["lam"][0] > 0.0 and rel < 1e-12
    assert cold_new["lam"][1] > 0.0 and cold_new["lam"][2] > 0.0         # vertex and third level
    for a, b in zip(new["solves"], old["solves"]):
        print("   iterations %d / %d, true residual %.6e / %.6e" % (a["iters"], b["iters"], a["true_res"], b["true_res"]))
        assert a["iters"] == b["iters"]
        assert a["rel"] <= 1e-12 and b["rel"] <= 1e-12
        assert abs(a["true_res"] - b["true_res"]) <= 1e-3 * b["true_res"]
        assert a["lam"][3] is True and b["lam"][3] is False              # the warm products too
