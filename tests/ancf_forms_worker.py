"""Worker, configuration table and judge of tests/test_gpu_ancf_forms.py: the element stage of the ANCF-3243 beam and the
ANCF-3443 shell (host mass values and ds/du, residual_kernel<8,12> / <16,48>, grad_kernel, tangent_blocks_kernel<8,12,6> /
<16,48,6>, assemble_rows_kernel<8> / <16>: csrc/elem_kernels.hip, csrc/data_api.hip) in one launch form per process -- the
library reads its TLFEA_* switches once.

    python tests/ancf_forms_worker.py '<json config>' <out.npz>

config: name, env (what the caller has put into the environment), cases, expect.  For every case (mesh, material,
options) the worker builds the data object as tests/test_gpu_ancf.py::make_pair does, sets the perturbed state of
tests/test_gpu_ancf.py::perturb with a velocity, asserts through tlfea_newton_get_assembly_form and the stage counters
that the launch form is the one the configuration is named for, and downloads det J, ds/du, the mass CSR, F and P at the
points, the internal force, the gradient and H with its index arrays, assembled twice.  It prints one JSON line and writes
the arrays to the npz; every comparison is the parent's, on the CPU, against orc.AncfOracle.

The module is imported by the CPU suite too (tests/test_ancf_edge_meshes.py): `case_inputs`, `oracle_reference` and the
judge functions need no GPU."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL_ELEM = 1e-12      # tests/test_gpu_parity.py: element-level quantities, relative to the largest entry
TOL_GEOM = 1e-13      # ... det J and the mass values
H_STEP, RHO = 1e-3, 1e12   # time step and penalty of tests/test_gpu_ancf.py::test_gradient_and_hessian
MATS = ("svk", "svk_damped", "mr_damped")     # SVK, SVK_D, MR_D of tests/test_gpu_ancf.py
WPB4 = {"TLFEA_TANGENT_WPB": "4"}


def case(mesh, mat, **opt):
    return dict(mesh=mesh, mat=mat, **opt)


def cases(mesh, mats=MATS, **opt):
    return [case(mesh, m, **opt) for m in mats]


DEFAULT_MESHES = ("one_beam", "one_shell", "chain5", "strip5", "fan3243_8", "fan3243_9", "fan3443_8", "fan3443_9",
                  "graded_chain5", "graded_strip5", "isolated_chain5", "isolated_strip5", "plate3443")
WPB4_MESHES = ("one_beam", "one_shell", "chain5", "strip5", "fan3243_9", "fan3443_9", "plate3443")
HUB_MESHES = ("fan3243_230", "fan3443_80")    # hub rows of 66 528 and 69 408 bytes of LDS in assemble_rows_kernel

# name, environment, cases, what the form query must report (check_expect)
CONFIGS = [("default_" + m, {}, cases(m), dict(wpb=1)) for m in DEFAULT_MESHES]
CONFIGS += [("wpb4_" + m, WPB4, cases(m), dict(wpb=4)) for m in WPB4_MESHES]
CONFIGS += [("default_" + m, {}, cases(m), dict(wpb=1, lds_over_64k=True)) for m in HUB_MESHES]
CONFIGS += [("hub_pinned_" + m, {}, cases(m, hub_pinned=True), dict(wpb=1, lds_over_64k=True)) for m in HUB_MESHES]
CONFIGS += [("wpb4_" + m, WPB4, cases(m, mats=("svk_damped", "mr_damped")), dict(wpb=4, lds_over_64k=True)) for m in HUB_MESHES]


# ---- inputs, shared by the worker and the judge -------------------------------------------------------------------------
def materials():
    import tests.test_gpu_ancf as A
    return {"svk": A.SVK, "svk_damped": A.SVK_D, "mr_damped": A.MR_D}


def mesh_of(name):
    """the 8-tuple of tests/ancf_edge_meshes.py and the coefficients the case pins"""
    from tests import ancf_edge_meshes as am
    if name == "plate3443":
        import tests.test_gpu_ancf as A
        kind, x, y, z, conn, (L, W, H), fixed, _ = A.plate_problem()
        E = conn.shape[0]
        return (kind, x, y, z, conn, np.full(E, L), np.full(E, W), np.full(E, H)), np.asarray(fixed, dtype=np.int32)
    m = am.build(name)
    if name.startswith("fan"):
        fixed = am.node_coefficients(1)              # the hub (node 0) is pinned only where the configuration says so
    elif m[0] == 3243:
        fixed = am.node_coefficients(0)
    else:
        fixed = am.node_coefficients([0, 1])         # the left edge of the strip
    if name.startswith("isolated_"):
        fixed = np.concatenate([fixed, am.node_coefficients(am.unused_nodes(m)[0])]).astype(np.int32)
    return m, fixed


def hub_of(conn):
    """the mesh node of the most elements (the lowest such node)"""
    nodes, counts = np.unique(conn, return_counts=True)
    return int(nodes[np.argmax(counts)])


def case_inputs(c):
    """everything both sides need: mesh, pinned coefficients, state (tests/test_gpu_ancf.py::perturb: the same draws), loads"""
    from tests import ancf_edge_meshes as am
    m, fixed = mesh_of(c["mesh"])
    kind, x, y, z, conn, L, W, H = m
    hub = hub_of(conn)
    if c.get("hub_pinned"):
        assert c["mesh"].startswith("fan") and hub == 0
        fixed = np.sort(np.concatenate([fixed, am.node_coefficients(hub)])).astype(np.int32)
    N = len(x)
    rng = np.random.default_rng(5)
    xs = [np.asarray(a, dtype=np.float64) + rng.normal(0, 1e-3, N) for a in (x, y, z)]
    v = rng.normal(0, 0.1, 3 * N)
    f_ext = np.random.default_rng(7).normal(0, 1e3, 3 * N)
    return dict(mesh=m, fixed=np.ascontiguousarray(fixed, dtype=np.int32), xs=xs, v=v, vp=0.3 * v, f_ext=f_ext,
                material=materials()[c["mat"]], hub=hub, last=conn[-1].astype(np.int64), N=N)


def problem_of(inp):
    """the tuple tests/test_gpu_ancf.py::make_pair takes"""
    kind, x, y, z, conn, L, W, H = inp["mesh"]
    return kind, x, y, z, conn, (L, W, H), inp["fixed"], inp["f_ext"]


def make_oracle(inp):
    from oracle import orc
    kind, x, y, z, conn, L, W, H = inp["mesh"]
    m = inp["material"]
    if m["kind"] == "svk":
        mat = orc.svk(m["E"], m["nu"], rho0=m["rho0"], eta=m["eta"], lamd=m["lamd"])
    else:
        mat = orc.mooney_rivlin(m["mu10"], m["mu01"], m["kappa"], rho0=m["rho0"], eta=m["eta"], lamd=m["lamd"])
    o = orc.AncfOracle(kind, x, y, z, conn, L, W, H, mat, inp["fixed"], inp["f_ext"])
    o.calc_dsdu_pre()
    o.calc_mass()
    return o


def oracle_reference(inp):
    """dict of the oracle's results on the inputs of case_inputs: det J, ds/du, mass CSR, F, P, f_int, grad L, H"""
    o = make_oracle(inp)
    r = dict(detJ=o.detJ.copy(), dsdu=o.gradN_a_d().copy(), m_off=o.m_off, m_col=o.m_col, m_val=o.m_val)
    o.x, o.y, o.z = (a.copy() for a in inp["xs"])
    o.v, o.v_prev = inp["v"].copy(), inp["vp"].copy()
    F, P = o.compute_p(None)
    # F and P of the points in the engine's layout ([E, Q, 3, 3], row-major F)
    r["F"] = F.reshape(-1, o.Q, 3, 3).transpose(0, 1, 3, 2)
    r["P"] = P.reshape(-1, o.Q, 3, 3).transpose(0, 1, 3, 2)
    r["f_int"] = o.internal_force(None)
    r["g"] = o.grad_L(o.internal_force(inp["v"]), H_STEP, RHO)
    r["ro"], r["ci"], r["val"] = o.assemble_hessian(H_STEP, RHO)
    return r


# ---- the judge (CPU only) -------------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0 and b.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def node_row_slots(ro, nodes):
    """indices into the CSR values of the 12 rows of H of every mesh node of `nodes` (four coefficients, three rows each)"""
    rows = (12 * np.atleast_1d(np.asarray(nodes, dtype=np.int64))[:, None] + np.arange(12)[None, :]).reshape(-1)
    return np.concatenate([np.arange(ro[r], ro[r + 1]) for r in rows]) if len(rows) else np.zeros(0, dtype=np.int64)


def judge_hessian(ro, ci, val, ro_ref, ci_ref, val_ref, val_again=None, hub=None, last=None, who=""):
    """H against the reference: index arrays bit-equal, values to TOL_ELEM of max|H|, the second assembly the same bits,
    symmetric to TOL_ELEM max|H|; the rows of the hub node alone and those of the last element's nodes alone to TOL_ELEM of
    the largest entry of those rows (the largest entry of H can be a pinned penalty elsewhere).  Returns the three relative
    errors (whole, hub rows, last element's rows); raises AssertionError."""
    import scipy.sparse as sp
    assert np.array_equal(ro, ro_ref) and np.array_equal(ci, ci_ref), (who, "index arrays differ from the oracle's")
    err = relerr(val, val_ref)
    assert err < TOL_ELEM, (who, "H", err)
    views = []
    for tag, nodes in (("hub rows", hub), ("last element's rows", last)):
        if nodes is None:
            views.append(0.0)
            continue
        k = node_row_slots(ro, nodes)
        assert k.size > 0, (who, tag, "no entries")
        views.append(relerr(val[k], val_ref[k]))
        assert views[-1] < TOL_ELEM, (who, "H", tag, views[-1])
    if val_again is not None:
        assert np.array_equal(val, val_again), (who, "the second assembly differs from the first")
    n = len(ro) - 1
    H = sp.csr_matrix((val, ci, ro), shape=(n, n))
    asym = abs(H - H.T).max() if H.nnz else 0.0
    assert asym < TOL_ELEM * np.max(np.abs(val)), (who, "H is not symmetric", float(asym))
    return err, views[0], views[1]


def judge_case(inp, ref, data, who=""):
    """every downloaded quantity of one case against the oracle's; returns the worst relative error of each"""
    err = {k: relerr(data[a], ref[k]) for k, a in (("detJ", "detJ"), ("m_val", "m_val"), ("dsdu", "dsdu"), ("F", "F"), ("P", "P"),
                                                    ("f_int", "f_int"), ("g", "g"))}
    assert np.array_equal(data["m_off"], ref["m_off"]) and np.array_equal(data["m_col"], ref["m_col"]), (who, "mass pattern")
    assert err["detJ"] < TOL_GEOM and err["m_val"] < TOL_GEOM, (who, err)
    for k in ("dsdu", "F", "P", "f_int", "g"):
        assert err[k] < TOL_ELEM, (who, k, err)
    err["H"], err["H_hub"], err["H_last"] = judge_hessian(data["H_ro"], data["H_ci"], data["H_val"], ref["ro"], ref["ci"], ref["val"],
                                                          data["H_val2"], inp["hub"], inp["last"], who)
    return err


# ---- what every configuration must report -----------------------------------------------------------------------------------
def check_expect(name, expect, form, stages, maxdeg, n_coef, gradient_form):
    """on the answers of tlfea_newton_get_assembly_form / _get_gradient_form and the stage counters of one assembly"""
    assert gradient_form == 1, (name, gradient_form)               # the mass CSR product inside grad_kernel
    assert form["mode"] == 1, (name, form)                         # tangent blocks, then one workgroup per coefficient row
    assert form["tangent_wpb"] == expect["wpb"], (name, form)
    assert form["lds_bytes"] == 9 * 8 * maxdeg, (name, form, maxdeg)
    assert (form["lds_bytes"] > 65536) == bool(expect.get("lds_over_64k")), (name, form)
    assert form["workgroups"] == n_coef and form["groups"] == n_coef, (name, form, n_coef)
    assert stages["tangent_blocks"][1] > 0 and stages["assemble_rows"][1] > 0, (name, stages)


# ---- the GPU side ---------------------------------------------------------------------------------------------------------
def run_case(c, tl):
    import tests.test_gpu_ancf as A
    inp = case_inputs(c)
    _, d = A.make_pair(problem_of(inp), inp["material"])
    out = dict(detJ=np.asarray(d.RetrieveDetJToCPU()), dsdu=np.asarray(d.RetrieveDsDuPreToCPU()))
    out["m_off"], out["m_col"], out["m_val"] = (np.asarray(a) for a in d.RetrieveMassCSRToCPU())
    d.UpdatePositions(*(a.copy() for a in inp["xs"]))
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 0.0, 1e-6, RHO, 5, 10, H_STEP))
    s.SetVelocity(inp["v"], inp["vp"])
    d.CalcP()                    # the elastic stress; the viscous part enters through the gradient below
    d.CalcInternalForce()
    out["F"], out["P"] = np.asarray(d.RetrieveDeformationGradientToCPU()), np.asarray(d.RetrievePFromFToCPU())
    out["f_int"] = np.asarray(d.RetrieveInternalForceToCPU()).copy()
    s.AnalyzeHessianSparsity()
    form = s.GetAssemblyForm()
    gform = s.GetGradientForm()
    s.SetProfiling(True)
    s.GetStageMs(reset=True)
    s.EvalGradient()
    out["g"] = s.RetrieveGradientToCPU()
    s.AssembleHessian()
    stages = s.GetStageMs(reset=True)
    s.SetProfiling(False)
    out["H_ro"], out["H_ci"], out["H_val"] = s.RetrieveHessianCSRToCPU()
    s.AssembleHessian()
    out["H_val2"] = s.RetrieveHessianCSRToCPU()[2]
    assert s.GetAssemblyForm() == form, (form, s.GetAssemblyForm())
    del s
    d.Destroy()
    return inp, form, stages, out, gform


def main(cfg, out_path):
    from tests.helpers import tl
    arrays, report = {}, []
    for k, c in enumerate(cfg["cases"]):
        inp, form, stages, out, gform = run_case(c, tl)
        check_expect(cfg["name"], cfg["expect"], form, stages, int(np.diff(out["m_off"]).max()), inp["N"], gform)
        arrays.update({"c%d_%s" % (k, key): v for key, v in out.items()})
        report.append(dict(case=c, form=form, gradient_form=gform, stage_counts={key: v[1] for key, v in stages.items()}, N=inp["N"],
                           E=int(out["detJ"].shape[0])))
    np.savez(out_path, **arrays)
    print(json.dumps(dict(name=cfg["name"], cases=report)), flush=True)


if __name__ == "__main__":
    cfg = json.loads(sys.argv[1])
    for key, v in cfg["env"].items():
        assert os.environ.get(key) == v, "the caller did not set %s=%s" % (key, v)
    main(cfg, sys.argv[2])
