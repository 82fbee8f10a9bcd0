"""Compact row form of the matrix-free Hessian product (csrc/matfree_compact.h): a wavefront of 64 elements sums
its element rows per node before it stores them, and the gather adds a node's compact rows in ascending wavefront order.

Same operator to rounding as the CSR product and as the element-row form (TLFEA_MATFREE_COMPACT=0): 1e-12 max |H p|, the
bound of tests/test_gpu_matfree.py and tests/cg_np.py.  Bit-identical from call to call, exact zeros in the p.q slots
beyond the gather's grid, and a forced-on linear solve takes as many CG iterations as the CSR solve and reaches the
requested tolerance on the true residual.

Meshes (tests/matfree_compact_worker.py): under one wavefront; 4 x 64 + 14 elements with 49 pinned nodes; a permuted
element order where nodes have up to 15 compact rows, so the gather's 8-lane loop makes a second trip.  The switches are
read once per process: every (mesh, switches) pair runs once in a fresh child, shared by the tests below.

Measured on MI355X: compact against CSR 1e-16 ... 5.5e-16, against the element rows 1e-20 ... 1.4e-16 (x max |H p|); solves
in 9, 16 and 19 iterations like the CSR solves, true residuals 8.2e-13, 6.4e-13, 4.6e-13 (profiles/r16_matfree_compact.txt)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12          # product bound, relative to max |H p|
REL_TOL = 1e-12      # requested tolerance of the solve (matfree_worker.REL_TOL)
NPART = 512
MESHES = ["small", "box", "permuted"]
_runs = {}


def run(mesh, matfree, compact, tmp_path_factory):
    key = (mesh, matfree, compact)
    if key not in _runs:
        npz = str(tmp_path_factory.mktemp("mfc") / "out.npz")
        env = dict(os.environ, TLFEA_SPMV_MATFREE=matfree, TLFEA_MATFREE_COMPACT=compact)
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "tests.matfree_compact_worker", mesh, npz],
                           cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        print(r.stdout.strip().splitlines()[-1])
        _runs[key] = dict(np.load(npz))
    return _runs[key]


def rel_err(y, ref):
    return float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("mesh", MESHES)
def test_product(mesh, tmp_path_factory):
    # with the CSR product in the Newton iterations that lead to H, both children assemble the same H bit for bit
    new = run(mesh, "0", "1", tmp_path_factory)
    old = run(mesh, "0", "0", tmp_path_factory)     # the element-row form (and the CSR solve of the test below)
    E = int(new["E"])
    assert int(new["form"]) == 1 and int(old["form"]) == 0
    assert int(old["rows"]) == 10 * E and int(new["rows"]) < 10 * E and float(new["ratio"]) == 10 * E / int(new["rows"])
    assert {"small": E < 64, "box": E % 64 != 0 and int(new["n_fixed"]) > 1, "permuted": E > 8 * 64}[mesh]
    for j in range(new["y"].shape[0]):
        ref = new["y_csr"][j]
        assert np.array_equal(ref, old["y_csr"][j])                   # same H in both children
        e_csr, e_old = rel_err(new["y"][j], ref), float(np.max(np.abs(new["y"][j] - old["y"][j])) / np.max(np.abs(ref)))
        print(f"{mesh} vector {j}: compact vs CSR {e_csr:.3e}, compact vs element rows {e_old:.3e}, "
              f"element rows vs CSR {rel_err(old['y'][j], ref):.3e}   (x max |H p|)")
        assert e_csr <= TOL and e_old <= TOL, (j, e_csr, e_old)
        assert np.array_equal(new["y"][j], new["y_again"][j]), j      # bitwise reproducible


@pytest.mark.parametrize("mesh", MESHES)
def test_product_in_the_forced_on_process(mesh, tmp_path_factory):
    """the state the pair itself led to: against the CSR product of that H, bitwise repeatable, and the raw p.q slots of two
    traced CG iterations hold exact zeros beyond the gather's grid"""
    new = run(mesh, "1", "1", tmp_path_factory)
    assert int(new["form"]) == 1 and int(new["trace_matfree"]) == 1
    for j in range(new["y"].shape[0]):
        e_csr = rel_err(new["y"][j], new["y_csr"][j])
        print(f"{mesh} vector {j}: compact vs CSR {e_csr:.3e} x max |H p|")
        assert e_csr <= TOL, (j, e_csr)
        assert np.array_equal(new["y"][j], new["y_again"][j]), j
    grid = max(1, min(NPART, math.ceil(int(new["N"]) / 128)))
    assert np.any(new["slots"][1:, 2, :grid] != 0.0) and not np.any(new["slots"][:, 2, grid:] != 0.0)


@pytest.mark.parametrize("mesh", MESHES)
def test_forced_on_solve_matches_the_csr_solve(mesh, tmp_path_factory):
    new = run(mesh, "1", "1", tmp_path_factory)
    csr = run(mesh, "0", "0", tmp_path_factory)
    assert int(new["mode"]) == 1 and int(csr["mode"]) == 0
    x_err = float(np.max(np.abs(new["x"] - csr["x"])) / np.max(np.abs(csr["x"])))
    print(f"{mesh}: iterations {int(new['iters'])} (CSR {int(csr['iters'])}), recurrence residual {float(new['rel']):.3e}, "
          f"true residual {float(new['true_res']):.6e} (CSR {float(csr['true_res']):.6e}), x_err {x_err:.3e}")
    assert int(new["iters"]) == int(csr["iters"])
    assert float(new["rel"]) <= REL_TOL and float(new["true_res"]) <= REL_TOL
    assert x_err <= 1e-10           # the displacement parity bound of the suite
