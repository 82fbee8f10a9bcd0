"""The T10 element stage -- mass values, residual, gradient, tangent and assembly kernels of csrc/elem_kernels.hip with
their host set-up (csrc/rowgroup_host.h, the sparsity code of csrc/tlfea_api.hip) -- in every launch form, on the meshes of
tests/edge_meshes.py: one element, element counts around a multiple of 64, a hub row that needs more than 64 KiB of LDS,
nodes of no element, a curved element.  Each configuration of tests/elem_forms_worker.py runs in a child process (the
library reads its switches once), one child at a time; the worker asserts the launch form through
tlfea_newton_get_assembly_form and the stage counters, this file judges every downloaded number on the CPU against the
oracle on the same inputs -- never with the project's own kernels.

Bounds (tests/test_gpu_parity.py): index arrays bit-equal; mass and det J to 1e-13, F, P, f_int, the gradient and H to
TOL_ELEM = 1e-12 of the largest entry; the second assembly the same bits; H symmetric to 1e-12 max|H| up to 600 nodes.
The hub row of star3 sums 512 element blocks: two fp64 summation orders of n terms differ by about 2 n eps of the sum
of magnitudes, 1.1e-13 here, inside TOL_ELEM.  Configurations that share mesh, material and state must agree with each
other to TOL_ELEM as well (affine, general, two-kernel; rolled, unrolled; default and changed budgets).  That the judge
rejects a wrong H is shown without a GPU in tests/test_edge_meshes.py.  Figures: profiles/elem_forms.txt, written by
running this file with TLFEA_ELEM_FORMS_REPORT=<file> (every line the tests print is then appended to that file too; the
variable is read here only, the children never see it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import orc
from tests import edge_meshes as em
from tests import elem_forms_worker as w
from tests.helpers import MATERIALS, fixed_x0, make_gpu, make_oracle, perturbed_state, relerr, tl
from tests.test_gpu_parity import disp_err_ok

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in w.CONFIGS]
# what the HIP runtime and the driver say when a kernel has faulted, in an error message of a child that did not die of a signal
GPU_FAULT_SIGNS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorIllegalAddress",
                   "hipErrorLaunchFailure", "unspecified launch failure", "HW Exception", "GPU Hang", "Aborted")


class Runs:
    """children run once each, strictly one at a time; oracle references once per case"""

    def __init__(self, tmp):
        self.tmp, self.done, self.refs = tmp, {}, {}

    def worker(self, name):
        if name in self.done:
            return self.done[name]
        _, env, cases, expect = next(c for c in w.CONFIGS if c[0] == name)
        npz = str(self.tmp / (name + ".npz"))
        cfg = dict(name=name, env=env, cases=cases, expect=expect)
        clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "elem_forms_worker.py"), json.dumps(cfg), npz], cwd=ROOT,
                               env=dict(clean, **env), capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % name, returncode=3)
        if r.returncode < 0 or r.returncode in (134, 139):  # killed by a signal: a GPU fault or an abort ends the session
            pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s" % (name, r.returncode, r.stderr[-3000:]),
                        returncode=3)
        if r.returncode != 0 and any(sign in r.stdout + r.stderr for sign in GPU_FAULT_SIGNS):
            # a fault the runtime reported as an error instead of a signal: the card is not to be used again either
            pytest.exit("%s: the worker met a GPU fault -- nothing more is started on this GPU\n%s" % (name, r.stderr[-3000:]), returncode=3)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        self.done[name] = (out, dict(np.load(npz, allow_pickle=False)))
        return self.done[name]

    def reference(self, c):
        key = json.dumps(c, sort_keys=True)
        if key not in self.refs:
            inp = w.case_inputs(c)
            self.refs[key] = (inp, w.oracle_reference(inp))
        return self.refs[key]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("elem_forms"))


def report(line):
    print(line)
    path = os.environ.get("TLFEA_ELEM_FORMS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def case_data(data, k):
    return {key[len("c%d_" % k):]: v for key, v in data.items() if key.startswith("c%d_" % k)}


@pytest.mark.parametrize("name", NAMES)
def test_elem_form(runs, name):
    out, data = runs.worker(name)
    expect = next(c for c in w.CONFIGS if c[0] == name)[3]
    for k, rec in enumerate(out["cases"]):
        c, form = rec["case"], rec["form"]
        inp, ref = runs.reference(c)
        d = case_data(data, k)
        who = "%s[%s %s]" % (name, c["mesh"], c["mat"])
        measured = {q: w.relerr(d[a], ref[b]) for q, a, b in (("detJ", "detJ", "detJ"), ("mass", "m_val", "m_val"), ("F", "F", "F"),
                                                              ("P", "P", "P"), ("f_int", "f_int", "f_int"), ("g", "g", "g"),
                                                              ("H", "H_val", "val"))} if d["H_val"].shape == ref["val"].shape else {}
        report("%-24s %-13s %-10s N %5d E %5d | mode %d rolled %d wpb %d G %5d acc_max %6d lds %6d wg %5d passes %6d | gradient form %d | "
               "stage counts tangent %d assemble %d | relerr %s"
               % (name, c["mesh"], c["mat"], rec["N"], rec["E"], form["mode"], form["rolled"], form["tangent_wpb"], form["groups"],
                  form["acc_max"], form["lds_bytes"], form["workgroups"], form["passes"], rec["gradient_form"], rec["stage_counts"]["tangent_blocks"],
                  rec["stage_counts"]["assemble_rows"], " ".join("%s %.1e" % kv for kv in measured.items())))
        w.judge_case(inp, ref, d, who)
        other = expect.get("more_groups_than")
        if other:
            base = runs.worker(other)[0]["cases"][k]["form"]
            assert form["groups"] > base["groups"] and form["mode"] == base["mode"], (who, form, base)


def test_forms_agree_with_each_other(runs):
    """configurations that share mesh, material, pinned nodes and state: their H agree to TOL_ELEM, whatever the form"""
    groups = {}
    for name in NAMES:
        out, data = runs.worker(name)
        for k, rec in enumerate(out["cases"]):
            groups.setdefault(json.dumps(rec["case"], sort_keys=True), []).append((name, rec["form"], case_data(data, k)["H_val"]))
    compared = 0
    for key, members in groups.items():
        for name, form, val in members[1:]:
            err = relerr(val, members[0][2])
            report("agree %-60s %-24s (mode %d) vs %-24s (mode %d): %.1e" % (key, name, form["mode"], members[0][0], members[0][1]["mode"], err))
            assert err < w.TOL_ELEM, (key, name, members[0][0], err)
            compared += 1
    modes = lambda key: {m[1]["mode"] for m in groups[json.dumps(key, sort_keys=True)]}
    assert modes(w.case("star3", "svk_damped")) == {1, 3} and modes(w.case("star3", "svk")) == {2, 3}     # over 64 KiB in each form
    assert modes(w.case("isolated_box", "svk")) == {1, 2, 3} and modes(w.case("bunny", "svk")) == {1, 2, 3}
    assert compared >= 12


# ---- in-process cases ----------------------------------------------------------------------------------------------------
def test_newton_refuses_nodes_of_no_element():
    """A solve with H is refused with the first such node and their number, before anything is launched; the same solver
    object still evaluates the gradient and assembles H, empty rows where the oracle has them."""
    X, conn, iso = em.isolated_box()
    m = MATERIALS["svk"]
    fixed = fixed_x0(X)
    assert iso[0] in fixed                                       # a pinned node of no element is among them
    o, d = make_oracle(X, conn, m, fixed), make_gpu(X, conn, m, fixed)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-4, 1e-4, w.RHO, 5, 10, w.H_STEP))
    s.SetProfiling(True)
    for lin in (tl.LinSolveOpts(1e-12, 2000, 10), tl.LinSolveOpts(method=1)):      # CG and direct
        s.SetLinSolveOpts(lin)
        calls = [s.Solve, s.NewtonIteration, lambda: s.LinearSolve(np.ones(3 * X.shape[0]))]
        if lin.method != 1:     # (the direct method has no preconditioner: that hook refuses it for this reason first)
            calls += [lambda: s.ApplyPreconditioner(np.ones(3 * X.shape[0])), lambda: s.ApplyPreconditioner(np.ones((2, 3 * X.shape[0])))]
        for call in calls:
            with pytest.raises(tl.TlfeaError, match=r"node 0 belongs to no element \(3 such nodes"):
                call()
    assert all(v[1] == 0 for v in s.GetStageMs().values())      # no stage ran
    s.SetProfiling(False)
    assert np.array_equal(np.stack(d.RetrievePositionToCPU(), axis=1), X)
    s.AssembleHessian()
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    ro_o, ci_o, val_o = o.assemble_hessian(w.H_STEP, w.RHO)
    w.judge_hessian(X.shape[0], ro, ci, val, ro_o, ci_o, val_o, who="after the refusal")
    assert np.all(np.diff(ro).reshape(-1, 3)[iso] == 0)
    # with H assembled, empty rows and all: whatever would invert its diagonal blocks is still refused, every hook included
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 2000, 10))
    s.SetProfiling(True)
    s.GetStageMs(reset=True)
    for call in (lambda: s.ApplyPreconditioner(np.ones(3 * X.shape[0])), lambda: s.ApplyPreconditioner(np.ones((2, 3 * X.shape[0]))),
                 lambda: s.LinearSolve(np.ones(3 * X.shape[0])), s.Solve):
        with pytest.raises(tl.TlfeaError, match=r"node 0 belongs to no element \(3 such nodes"):
            call()
    assert all(v[1] == 0 for v in s.GetStageMs().values())
    assert "VBD" not in tl.load_library().tlfea_last_error().decode()
    del s
    v = tl.SyncedVBDSolver(d, d.get_n_constraint())             # the vertex solve reads a diagonal mass entry such a node lacks
    v.SetParameters(tl.SyncedVBDParams(max_outer=1, max_inner=5))
    with pytest.raises(tl.TlfeaError, match=r"node 0 belongs to no element \(3 such nodes"):
        v.Solve()
    assert np.array_equal(np.stack(d.RetrievePositionToCPU(), axis=1), X)
    del v
    d.Destroy()


def test_adamw_keeps_nodes_of_no_element_inert():
    """AdamW never forms H: zero gradient and zero mass leave such a node exactly where it was, the rest of the mesh
    follows the oracle's AdamW (tests/test_gpu_ancf.py: tolerances that cannot trigger, every coordinate perturbed)."""
    X, conn, iso = em.isolated_box()
    m = MATERIALS["svk_damped"]
    f_ext = np.random.default_rng(5).normal(0, 1e3, 3 * X.shape[0])
    f_ext.reshape(-1, 3)[iso] = 0.0
    o, d = make_oracle(X, conn, m, None, f_ext), make_gpu(X, conn, m, None, f_ext)
    x0, _ = perturbed_state(X, sigma=1e-4)
    o.x, o.y, o.z = (np.ascontiguousarray(x0[:, i]) for i in range(3))
    d.UpdatePositions(x0[:, 0].copy(), x0[:, 1].copy(), x0[:, 2].copy())
    kw = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, lr_decay=0.998, inner_tol=0.0, outer_tol=0.0,
              rho=1e14, max_outer=1, max_inner=40, time_step=1e-3, convergence_check_interval=10, inner_rtol=0.0)
    s = tl.SyncedAdamWNocoopSolver(d, 0)
    s.Setup()
    s.SetParameters(tl.SyncedAdamWNocoopParams(**kw))
    s.Solve()
    o.S, o.Q = 10, 5
    st_o = orc.ElemOracle.adamw_step(o, orc.AdamWParams(*[kw[k] for k, _ in orc.AdamWParams._fields_]))
    st_g = s.GetStats()
    assert (st_g["outer"], st_g["inner"], st_g["inner_flag"]) == (int(st_o[0]), int(st_o[1]), int(st_o[4])) == (1, 40, 0)
    xg = np.stack(d.RetrievePositionToCPU(), axis=1)
    xo = np.stack([o.x, o.y, o.z], axis=1)
    vg = s.RetrieveVelocityToCPU()
    assert np.array_equal(xg[iso], x0[iso]) and np.all(vg.reshape(-1, 3)[iso] == 0.0)      # bit for bit
    assert np.max(np.abs(xo - x0)) > 1e-6                       # the mesh did move
    assert disp_err_ok(xg, xo, x0), (np.max(np.abs(xg - xo)), np.max(np.abs(xo - x0)))
    assert relerr(vg, o.v) < 1e-10
    del s
    d.Destroy()


def test_star4_is_refused_before_any_launch():
    """The hub row of star4 needs 360 KiB of LDS in assemble_rows_kernel and more in the fused forms; the row-group
    builders accept it.  The sparsity analysis refuses it by the device's limit, names node, degree and limit, and leaves
    the solver object and the data object usable."""
    X, conn = em.build("star4")
    hub = em.star_hub(X, conn)
    d = make_gpu(X, conn, MATERIALS["svk"], None)
    s = tl.SyncedNewtonSolver(d, 0)
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-4, 1e-4, w.RHO, 5, 10, w.H_STEP))
    s.SetProfiling(True)
    msg = r"node %d has 5125 neighbours: its row of H needs 369000 bytes of LDS in the assembly, a workgroup of this device has \d+" % hub
    for call in (s.AnalyzeHessianSparsity, s.AssembleHessian, s.Solve, s.GetAssemblyForm):
        with pytest.raises(tl.TlfeaError, match=msg):
            call()
    assert all(v[1] == 0 for v in s.GetStageMs().values())
    del s
    x, _ = perturbed_state(X)
    d.UpdatePositions(x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy())
    d.CalcP()
    d.CalcInternalForce()
    o = make_oracle(X, conn, MATERIALS["svk"])
    o.x, o.y, o.z = (np.ascontiguousarray(x[:, i]) for i in range(3))
    assert relerr(d.RetrieveInternalForceToCPU(), o.internal_force(None)) < w.TOL_ELEM
    d.Destroy()


STAR3_STEP = (1e-6, 0.0, 1e-6, 1e14, 1, 1, 1e-3)      # one outer, one Newton iteration: one assembly and one linear solve


@pytest.fixture(scope="module")
def star3_step():
    """the loaded star3 with a free hub and the oracle's step on it (dense Cholesky of 3 855 unknowns: once for the three solves)"""
    inp = w.case_inputs(w.case("star3", "svk"))
    X, conn, fixed = inp["X"], inp["conn"], inp["fixed"]
    hub = em.star_hub(X, conn)
    assert hub not in fixed
    f_ext = np.zeros(3 * X.shape[0])
    f_ext[3 * hub + 2] = 2.0e5
    far = np.where(X[:, 0] > 0.9)[0]
    f_ext[3 * far] = 5.0e4 / len(far)
    o = make_oracle(X, conn, MATERIALS["svk"], fixed, f_ext)
    o.newton_step(orc.NewtonParams(*STAR3_STEP), solver=0)
    return X, conn, fixed, hub, f_ext, np.stack([o.x, o.y, o.z], axis=1)


@pytest.mark.parametrize("solve", ["pmg", "polynomial", "direct"])
def test_newton_step_on_star3_with_a_free_hub(star3_step, solve):
    """One implicit step on star3, the hub free: its row of H has 3 855 entries, the longest the row-sweep kernels of the
    linear solve see in a test.  Displacements against the oracle's step (dense Cholesky), bar of tests/test_gpu_parity.py."""
    X, conn, fixed, hub, f_ext, xo = star3_step
    d = make_gpu(X, conn, MATERIALS["svk"], fixed, f_ext)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(*STAR3_STEP))
    if solve == "direct":
        s.SetLinSolveOpts(tl.LinSolveOpts(method=1))
    else:
        pre = 2 if solve == "pmg" else 1
        s.SetLinSolveOpts(tl.LinSolveOpts(1e-13, 20000, 10, 0, 0.0, 0, pre))
        assert s.GetPreconditioner() == pre
    s.Solve()
    ro, _, _ = s.RetrieveHessianCSRToCPU()
    assert ro[3 * hub + 1] - ro[3 * hub] == 3855
    xg = np.stack(d.RetrievePositionToCPU(), axis=1)
    disp = np.max(np.abs(xo - X))
    report("newton_star3 %-10s stats %s max |x_gpu - x_oracle| %.3e displacement %.3e (hub %.3e)"
           % (solve, s.GetStats(), np.max(np.abs(xg - xo)), disp, np.max(np.abs(xo[hub] - X[hub]))))
    assert s.GetStats()["newton"] == 1
    assert disp > 1e-4 and np.max(np.abs(xo[hub] - X[hub])) > 1e-5      # the relative bar is exercised, at the hub too
    assert disp_err_ok(xg, xo, X)
    if solve != "direct":
        assert s.GetPreconditioner() == pre
    del s
    d.Destroy()
