"""Packed, lane-major element records of the matrix-free passes (DESIGN 3g, 3g', csrc/matfree_records.h) on the device, with
four and with five stored points (TLFEA_MATFREE_POINTS).

The pack kernel writes what tests/matfree_records_np.py packs from the element-major records: bit for bit in fp64, and
float32(x) in the fine smoother's copy.  The fp64 product from the packed records is the CSR product of the same H to
1e-12 max |H p| (the suite's bound: tests/test_gpu_matfree.py), bit-identical from call to call, in the compact row form
and in the element-row form; a forced-on solve takes as many CG iterations as the CSR solve and reaches the tolerance on
the true residual.  One fine smoother pass stays within the bound of tests/test_gpu_fine_matfree.py, min(8 x the CPU's
float32 floor, 1e-4).  After another assembly the product reads the new generation of records, and a smoother pass
against the old one is refused.

Meshes (tests/matfree_compact_worker.py): under one wavefront; 4 x 64 + 14 elements with 49 pinned nodes; a permuted
element order.  The switches are read once per process: every (mesh, switches) pair runs once in a fresh child, shared by
the tests below.

Measured on MI355X: product against CSR 1.1e-19 ... 9.5e-16 with five points, 1.1e-19 ... 8.2e-16 with four (x max |H p|);
solves in 9, 16 and 19 iterations like the CSR solves, true residuals 8.4e-13, 5.6e-13, 4.5e-13; smoother pass 1.7e-7 ...
8.5e-7 against floors of 1.6e-7 ... 4.6e-7 (profiles/matfree_records.txt)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fine_matfree_np as fm
from tests import matfree_records_np as rn
from tests import precond_np as pn
from tests import test_gpu_fine_matfree as tgf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12          # product bound, relative to max |H p|
REL_TOL = 1e-12      # requested tolerance of the solve (matfree_worker.REL_TOL)
MESHES = ["small", "box", "permuted"]
POINTS = [4, 5]
STALE = "the records have changed since"
_runs = {}


def run(mesh, points, matfree, compact, tmp_path_factory):
    key = (mesh, points, matfree, compact)
    if key not in _runs:
        npz = str(tmp_path_factory.mktemp("mfr") / "out.npz")
        clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
        env = dict(clean, TLFEA_MATFREE_POINTS=str(points), TLFEA_SPMV_MATFREE=matfree, TLFEA_MATFREE_COMPACT=compact,
                   TLFEA_PMG_FINE_MATFREE="1")
        try:
            r = subprocess.run([sys.executable, "-m", "tests.matfree_records_worker", mesh, npz], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % (key,), returncode=3)
        if r.returncode < 0 or r.returncode in (134, 139):
            pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s" % (key, r.returncode, r.stderr[-3000:]),
                        returncode=3)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        print(r.stdout.strip().splitlines()[-1])
        _runs[key] = dict(np.load(npz))
    return _runs[key]


def rel_err(y, ref):
    return float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("points", POINTS)
@pytest.mark.parametrize("mesh", MESHES)
def test_read_back_is_the_numpy_pack(mesh, points, tmp_path_factory):
    o = run(mesh, points, "1", "1", tmp_path_factory)
    E = int(o["E"])
    assert {"small": E < 64, "box": E % 64 == 14 and E // 64 == 4, "permuted": E > 8 * 64}[mesh]
    assert int(o["points64"]) == points and int(o["fine"]) == 1 and int(o["points32"]) == points
    assert o["gvec"].shape == (E, 16) and o["Fq"].shape == (E, 5, 10)
    gp, Fp = rn.pack(o["gvec"], o["Fq"], points, np.float64)
    assert o["gp64"].dtype == np.float64 and np.array_equal(o["gp64"], gp) and np.array_equal(o["Fp64"], Fp)     # bit for bit
    gp32, Fp32 = rn.pack(o["gvec"], o["Fq"], points, np.float32)
    assert o["gp32"].dtype == np.float32 and np.array_equal(o["gp32"], gp32) and np.array_equal(o["Fp32"], Fp32)  # float32(x)
    assert np.abs(o["Fq"][:, :, :9].reshape(E, 5, 3, 3) - np.eye(3)).max() > 1e-4                                # F differs from I


@pytest.mark.parametrize("compact", ["1", "0"])
@pytest.mark.parametrize("points", POINTS)
@pytest.mark.parametrize("mesh", MESHES)
def test_product(mesh, points, compact, tmp_path_factory):
    o = run(mesh, points, "1" if compact == "1" else "0", compact, tmp_path_factory)
    assert int(o["form"]) == int(compact) and int(o["points64"]) == points
    for j in range(o["y"].shape[0]):
        e = rel_err(o["y"][j], o["y_csr"][j])
        print(f"{mesh} {points} points compact={compact} vector {j}: packed records vs CSR {e:.3e} x max |H p|")
        assert e <= TOL, (j, e)
        assert np.array_equal(o["y"][j], o["y_again"][j]), j            # bitwise reproducible


@pytest.mark.parametrize("points", POINTS)
@pytest.mark.parametrize("mesh", MESHES)
def test_forced_on_solve_matches_the_csr_solve(mesh, points, tmp_path_factory):
    new = run(mesh, points, "1", "1", tmp_path_factory)
    csr = run(mesh, points, "0", "0", tmp_path_factory)
    assert int(new["mode"]) == 1 and int(csr["mode"]) == 0
    x_err = float(np.max(np.abs(new["x"] - csr["x"])) / np.max(np.abs(csr["x"])))
    print(f"{mesh} {points} points: iterations {int(new['iters'])} (CSR {int(csr['iters'])}), recurrence residual "
          f"{float(new['rel']):.3e}, true residual {float(new['true_res']):.6e}, x_err {x_err:.3e}")
    assert int(new["iters"]) == int(csr["iters"])
    assert float(new["rel"]) <= REL_TOL and float(new["true_res"]) <= REL_TOL
    assert x_err <= 1e-10           # the displacement parity bound of the suite


@pytest.mark.parametrize("points", POINTS)
@pytest.mark.parametrize("mesh", MESHES)
def test_generations(mesh, points, tmp_path_factory):
    o = run(mesh, points, "1", "1", tmp_path_factory)
    assert not np.array_equal(o["Fq2"], o["Fq"]) and not np.array_equal(o["y2_csr"], o["y_csr"][0])   # H has moved
    e = rel_err(o["y2"], o["y2_csr"])
    print(f"{mesh} {points} points: product of the next generation vs its CSR product {e:.3e} x max |H p|")
    assert e <= TOL
    assert np.array_equal(o["Fp2"], rn.pack(o["gvec"], o["Fq2"], points, np.float64)[1])
    assert STALE in str(o["stale"]), o["stale"]


@pytest.mark.parametrize("points", POINTS)
@pytest.mark.parametrize("mesh", ["beam_3x2x1", "box", "permuted"])
def test_one_smoother_pass(mesh, points, tmp_path):
    """the scenario and the bound of tests/test_gpu_fine_matfree.py::test_one_pass_in_each_coefficient_form"""
    out, data = tgf.run(dict(what="operator", mesh=mesh), dict(tgf.ON, TLFEA_MATFREE_POINTS=str(points)), tmp_path,
                        "%s_%d" % (mesh, points))
    assert out["fine_smoother"] == 1
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
        print(mesh, points, nm, " ".join("%s: floor %.2e device %.2e" % (k, f, o[k]) for k, f in floors.items()))
        assert o["finite"] and o["bitwise"], (nm, o)
        for k, f in floors.items():
            assert 0.0 < f <= 1e-4, (nm, k, f)
            assert o[k] <= min(8.0 * f, 1e-4), (nm, k, o[k], f)
