"""Every kernel regime of the native sparse direct solve (LinSolveOpts(method=1): csrc/mf_host.h, csrc/direct_kernels.hip)
pinned as an operator on small meshes: the stack regime, the 128-tile trailing update, the step-by-step triangular solves,
super-panels of every length -- each forced through the TLFEA_DIRECT_* switches on a mesh of at most 12 675 DOF.  Each
configuration runs tests/direct_worker.py in a child process (the library reads its switches once), one child at a time; the
worker asserts that the launches the library counted are the ones its regime consists of (tests/direct_worker.py,
check_expect), this file judges the numbers, on the CPU, from the H the worker downloaded -- never with the project's own
SpMV.

Bounds.  Measured, against references only: for each configuration's H two fp64 sparse LU solves with different
elimination orders (scipy splu, COLAMD and MMD_AT_PLUS_A).  eta = ||b - Hx|| / (||H||_F ||x|| + ||b||), residuals in
long double; eta_ref is the larger of the two references' eta and fwd_ref their relative distance, each the maximum over
the right-hand sides.  The device must keep eta <= 10 max(eta_ref, 2.2e-16) and
||x - x_ref|| / ||x_ref|| <= 10 max(fwd_ref, 2.2e-16 sqrt(n)): the factor 10 is what separates two backward-stable fp64
factorisations of one matrix (summation order, FMA contraction); a dropped or doubled tile, panel column or child
contribution leaves eta many orders above it.  A configuration whose fwd_ref exceeds 1e-6 fails: its matrix is to be made
better conditioned, not the bound wider.

stack_0 / stack_2 / stack_all / levels_ref share ordering, extend-add order, panel arithmetic and (TLFEA_DIRECT_WIDE_TILES
pinned) the tile kernel; the stack regime only moves update matrices, so their solutions are required to be bit-identical.

The worker solves with on_unconverged=1, so that a wrong solution is returned and judged here instead of being stopped
by the library's own 1e-8 residual guard (which measures with the library's own SpMV).

Where the configurations differ from a first reading of the meshes (all asserted in tests/direct_worker.py and, without
a GPU, in tests/test_direct_plan.py): the pair of boxes of test_direct_two_disconnected_bodies (441 + 315 nodes) does NOT
give an empty root front -- the median plane lies inside the first body -- so two_bodies_stack uses two equal boxes,
whose root separator is empty; res2 at the default leaf has no front below 48 rows, so stepwise_all pins panels narrower
than 48 columns and one-block grids, and fronts below 48 rows (and the front without own columns) are pinned by
stepwise_all_leaf4; the randomly perturbed ANCF plate of tests/precond_worker.py is indefinite at the 1e-3 time step (15
negative eigenvalues, CPU oracle), so ancf_plate runs at 1e-4.

Sanity of these tests: one-line in-bounds breaks of the stack path's c_ld, the 128-tile kernel's `in` mask and
mf_bwd_step_kernel's column guard in scratch builds each fail the configurations that reach them, eta six to nine orders
above bound (a); figures in profiles/direct_regimes.txt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import direct_worker as dw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.2e-16


class Runs:
    """children run once each, strictly one at a time; references once per matrix"""

    def __init__(self, tmp):
        self.tmp, self.done, self.refs = tmp, {}, {}

    def worker(self, name, problem, env, mode="solve"):
        if name in self.done:
            return self.done[name]
        npz = str(self.tmp / (name + ".npz"))
        cfg = dict(name=name, problem=problem, env=env, mode=mode)
        clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "direct_worker.py"), json.dumps(cfg), npz], cwd=ROOT,
                               env=dict(clean, **env), capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % name, returncode=3)
        if r.returncode < 0 or r.returncode in (134, 139):  # killed by a signal: a GPU fault or an abort ends the session
            pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s" % (name, r.returncode, r.stderr[-3000:]),
                        returncode=3)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        self.done[name] = (out, dict(np.load(npz, allow_pickle=False)))
        return self.done[name]

    def config(self, name):
        problem, env = {c[0]: c[1:] for c in dw.CONFIGS}[name]
        if name != "stack_auto":
            return self.worker(name, problem, env)
        ref = self.config("levels_ref")[0]["info"]
        for f in dw.STACK_AUTO_FRACTIONS:    # the first bound the plan accepts; none accepted: a failure, not a skip
            env = dw.stack_auto_env(ref, f)
            try:
                return self.worker(name, problem, env)
            except AssertionError as e:
                if "do not fit" not in str(e):
                    raise
        raise AssertionError("stack_auto: the plan accepts none of the memory bounds %r" % (dw.STACK_AUTO_FRACTIONS,))

    def references(self, key, H):
        """the two fp64 references of a matrix, factored once per problem (the configurations of a problem share H)"""
        if key not in self.refs or not np.array_equal(self.refs[key][0], H.data):
            Hc = H.tocsc()
            self.refs[key] = (H.data.copy(), spla.splu(Hc, permc_spec="COLAMD"), spla.splu(Hc, permc_spec="MMD_AT_PLUS_A"))
        return self.refs[key][1:]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("direct_regimes"))


def matrix(data):
    n = len(data["H_ro"]) - 1
    return sp.csr_matrix((data["H_val"], data["H_ci"], data["H_ro"]), shape=(n, n))


def residual_norm(H, x, b):
    """||b - H x||_2 accumulated in long double, from the CSR arrays (no library SpMV)"""
    ld = np.longdouble
    prod = H.data.astype(ld) * x.astype(ld)[H.indices]
    Hx = np.add.reduceat(prod, H.indptr[:-1])          # (every row of H has its diagonal: no empty row)
    return float(np.sqrt(np.sum((b.astype(ld) - Hx) ** 2)))


def eta(H, normF, x, b):
    den = normF * np.linalg.norm(x) + np.linalg.norm(b)
    return residual_norm(H, x, b) / den if den > 0 else 0.0


def judge(runs, key, data, tags):
    """(eta_ref, fwd_ref, eta_dev, fwd_dev, per-vector figures) of a worker's solutions"""
    H = matrix(data)
    assert np.all(np.diff(H.indptr) > 0)
    normF = float(np.sqrt(np.sum(H.data.astype(np.longdouble) ** 2)))
    lu1, lu2 = runs.references(key, H)
    eta_ref = fwd_ref = eta_dev = fwd_dev = 0.0
    per = {}
    for tag, b, x in zip(tags, data["B"], data["X"]):
        if not np.any(b):
            continue
        x1, x2 = lu1.solve(b), lu2.solve(b)
        e_ref = max(eta(H, normF, x1, b), eta(H, normF, x2, b))
        f_ref = float(np.linalg.norm(x1 - x2) / np.linalg.norm(x1))
        e, f = eta(H, normF, x, b), float(np.linalg.norm(x - x1) / np.linalg.norm(x1))
        per[tag] = dict(eta_ref=e_ref, fwd_ref=f_ref, eta=e, fwd=f, res_rel=residual_norm(H, x, b) / float(np.linalg.norm(b)))
        eta_ref, fwd_ref, eta_dev, fwd_dev = max(eta_ref, e_ref), max(fwd_ref, f_ref), max(eta_dev, e), max(fwd_dev, f)
    return eta_ref, fwd_ref, eta_dev, fwd_dev, per


def report(line):
    print(line)
    path = os.environ.get("TLFEA_DIRECT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("name", [c[0] for c in dw.CONFIGS])
def test_direct_regime(runs, name):
    out, data = runs.config(name)
    tags = [str(t) for t in data["tags"]]
    info = out["info"]
    n = out["n"]
    eta_ref, fwd_ref, eta_dev, fwd_dev, per = judge(runs, {c[0]: c[1] for c in dw.CONFIGS}[name], data, tags)
    eta_bound, fwd_bound = 10.0 * max(eta_ref, EPS), 10.0 * max(fwd_ref, EPS * np.sqrt(n))
    report("%-20s n %5d fronts %3d levels %2d top_depth %2d m_max %4d k_max %3d k_zero %d | panel %3d inner %3d trailing64 %3d "
           "wide128 %3d extend %3d push %3d | levels one-wg %2d stepwise %2d fwd/bwd steps %2d/%2d | eta_ref %.2e eta %.2e "
           "(bound %.2e)  fwd_ref %.2e fwd %.2e (bound %.2e)"
           % (name, n, info["fronts"], info["levels"], info["top_depth"], info["m_max"], info["k_max"], info["k_zero"],
              info["panel"], info["update_inner"], info["update_trailing"], info["update_wide"], info["extend_add"],
              info["push"], info["levels_one_wg"], info["levels_stepwise"], info["fwd_step"], info["bwd_step"], eta_ref,
              eta_dev, eta_bound, fwd_ref, fwd_dev, fwd_bound))
    print(json.dumps(per))
    assert fwd_ref <= 1e-6, (name, fwd_ref, "make this configuration's matrix better conditioned")
    assert np.all(np.isfinite(data["X"]))
    for tag in per:                                                                               # (a), (b)
        assert per[tag]["eta"] <= eta_bound, (name, tag, per[tag]["eta"], eta_bound)
        assert per[tag]["fwd"] <= fwd_bound, (name, tag, per[tag]["fwd"], fwd_bound)
    z = tags.index("b_zero")                                                                      # (c)
    assert not np.any(data["B"][z]) and np.all(data["X"][z] == 0.0) and data["rel"][z] == 0.0
    assert np.array_equal(data["X_first"], data["X"][tags.index("b_rand")])                       # (d) same bits
    # (e) the worker has required the counted launches to be those of the regime (it fails otherwise); the record it
    # judged is the one saved
    assert [int(v) for v in data["info"]] == [info[str(k)] for k in data["info_keys"]]
    assert np.all(data["it"] == 1)                                                                # (f)
    for tag, rel in zip(tags, data["rel"]):
        if tag in per:
            cpu = per[tag]["res_rel"]
            assert (rel < 1e-14 and cpu < 1e-14) or (cpu / 4 <= rel <= 4 * cpu), (name, tag, float(rel), cpu)


def test_stack_regime_has_the_bits_of_whole_levels(runs):
    """stack_0, stack_2, stack_all and levels_ref: same ordering, same extend-add order (child 0, then child 1), same panel
    and tile arithmetic -- the stack regime only copies update matrices (mf_push_kernel) and reads them through another
    leading dimension.  Their solutions are the same bits, for every right-hand side the plans share."""
    ref = runs.config("levels_ref")[1]
    tags = [str(t) for t in ref["tags"]]
    for name in ("stack_0", "stack_2", "stack_all"):
        data = runs.config(name)[1]
        assert np.array_equal(data["H_val"], ref["H_val"]) and np.array_equal(data["order"], ref["order"])
        for tag in ("b_rand", "b_ones", "b_leaf", "b_root"):
            i = tags.index(tag)
            assert np.array_equal(data["B"][i], ref["B"][i]), (name, tag)
            differ = int(np.sum(data["X"][i] != ref["X"][i]))
            assert differ == 0, (name, tag, differ, float(np.max(np.abs(data["X"][i] - ref["X"][i]))))


def test_indefinite_matrix_under_a_forced_regime_then_a_definite_one(runs):
    """A pivot that is not positive is reported in the stack regime with a trailing update after every panel, and the same
    solver object then solves the definite H within the bounds: the error flag and the workspaces start afresh."""
    env = {"TLFEA_DIRECT_TOP_DEPTH": "0", "TLFEA_DIRECT_SUPER": "1"}
    out, data = runs.worker("indefinite_then_definite", "res2", env, mode="indefinite")
    assert "not positive" in out["message"], out["message"]
    eta_ref, fwd_ref, eta_dev, fwd_dev, per = judge(runs, "res2_svk_unperturbed", data, ["b_rand"])
    n = data["B"].shape[1]
    report("%-20s n %5d eta_ref %.2e eta %.2e  fwd_ref %.2e fwd %.2e" % ("indefinite_then_ok", n, eta_ref, eta_dev, fwd_ref, fwd_dev))
    assert fwd_ref <= 1e-6
    assert eta_dev <= 10.0 * max(eta_ref, EPS) and fwd_dev <= 10.0 * max(fwd_ref, EPS * np.sqrt(n)), (eta_dev, eta_ref, fwd_dev, fwd_ref)
    assert data["it"][0] == 1


def test_plan_refusal_leaves_the_iterative_solver_usable(runs):
    """A factor that does not fit its bound is refused with the message that names the switch, and an iterative solve on
    the same solver object converges (judged by the CPU residual on the downloaded H)."""
    out, data = runs.worker("plan_refusal", "res2", {"TLFEA_DIRECT_MAX_NNZ": "1000"}, mode="refusal")
    assert "do not fit" in out["message"], out["message"]
    H = matrix(data)
    res = residual_norm(H, data["X"][0], data["B"][0]) / float(np.linalg.norm(data["B"][0]))
    report("%-20s iterative solve after the refusal: %d iterations, reported rel %.2e, CPU residual %.2e"
           % ("plan_refusal", out["it"], out["rel"], res))
    # the CG's own stopping test at rel_tol 1e-12; the true residual of the returned x may sit above the recurrence's by
    # cond(H) eps ||x|| ||H|| / ||b||: two orders are allowed for that
    assert out["rel"] <= 1e-12 and res <= 1e-10 and out["it"] > 1, (out, res)
