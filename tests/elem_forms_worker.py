"""Worker, configuration table and judge of tests/test_gpu_elem_forms.py: the T10 element stage (mass values, residual,
gradient, tangent, assembly: csrc/elem_kernels.hip, with the host set-up of csrc/rowgroup_host.h) in one launch form
per process -- the library reads its TLFEA_* switches once.

    python tests/elem_forms_worker.py '<json config>' <out.npz>

config: name, env (what the caller has put into the environment), cases, expect.  For every case (mesh, material,
options) the worker builds the mesh, sets the perturbed state of tests.helpers.perturbed_state, asserts through
tlfea_newton_get_assembly_form and the stage counters that the launch form is the one the configuration is named for (a
configuration that falls back to another form fails here), and downloads det J, the mass CSR, F and P at the points, the
internal force, the gradient (random f_ext, v, v_prev, pinned nodes) and H with its index arrays, assembled twice.  It
prints one JSON line and writes the arrays to the npz; every comparison is the parent's, on the CPU, against the oracle.

The module is imported by the CPU suite too (tests/test_edge_meshes.py): `case_inputs` and the judge functions need no GPU."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOL_ELEM = 1e-12      # tests/test_gpu_parity.py: element-level quantities, relative to the largest entry
TOL_GEOM = 1e-13      # ... det J and the mass values
H_STEP, RHO = 1e-3, 1e12   # time step and penalty of tests/test_gpu_parity.py::test_hessian
GENERAL, KBUF = {"TLFEA_ASSEMBLE": "general"}, {"TLFEA_ASSEMBLE": "kbuf"}

# per-element material tables (three entries; the oracle has one material per object: the parent sums one oracle per entry)
TABLES = {
    "svk": [dict(kind="svk", E=7e8, nu=0.33, rho0=2700.0, eta=1e5, lamd=2e5),
            dict(kind="svk", E=3e7, nu=0.45, rho0=900.0, eta=3e3, lamd=0.0),
            dict(kind="svk", E=2e9, nu=0.2, rho0=7800.0, eta=0.0, lamd=1e4)],
    "mr": [dict(kind="mr", mu10=4e7, mu01=1e7, kappa=5e8, rho0=920.0, eta=2e4, lamd=3e4),
           dict(kind="mr", mu10=2e6, mu01=5e5, kappa=4e7, rho0=1500.0, eta=0.0, lamd=1e3),
           dict(kind="mr", mu10=9e7, mu01=0.0, kappa=9e8, rho0=1100.0, eta=1e3, lamd=0.0)],
}


def case(mesh, mat, **opt):
    return dict(mesh=mesh, mat=mat, **opt)


# name, environment, cases, what the form query must report (check_expect)
CONFIGS = [
    ("affine_one_tet", {}, [case("one_tet", "svk")], dict(mode=3)),
    ("general_one_tet_mr", {}, [case("one_tet", "mr")], dict(mode=2)),
    ("affine_192", {}, [case("box_192", "svk_damped")], dict(mode=3)),
    ("affine_65", {}, [case("box_65", "svk_damped")], dict(mode=3)),
    ("affine_63", {}, [case("box_63", "svk_damped")], dict(mode=3)),
    ("affine_star2", {}, [case("star2", "svk")], dict(mode=3)),
    ("affine_star3", {}, [case("star3", "svk")], dict(mode=3, lds_over_64k=True)),
    ("affine_star3_hub_pinned", {}, [case("star3", "svk_damped", hub_pinned=True)], dict(mode=3, lds_over_64k=True)),
    ("general_star3", GENERAL, [case("star3", "svk")], dict(mode=2, rolled=1, lds_over_64k=True)),
    ("general_star3_curved", {}, [case("curved_star3", "svk_damped")], dict(mode=2, lds_over_64k=True)),
    ("general_star2_curved", {}, [case("curved_star2", "svk_damped")], dict(mode=2)),
    ("unrolled_star2", dict(GENERAL, TLFEA_AD_ROLLED="0"), [case("star2", "svk_damped")], dict(mode=2, rolled=0)),
    ("unrolled_bunny", dict(GENERAL, TLFEA_AD_ROLLED="0"), [case("bunny", "svk_damped")], dict(mode=2, rolled=0)),
    ("mr_star3", {}, [case("star3", "mr_damped")], dict(mode=2, lds_over_64k=True)),
    ("kbuf_star3", KBUF, [case("star3", "svk_damped")], dict(mode=1, stage2=True, lds_over_64k=True)),
    ("kbuf_bunny", KBUF, [case("bunny", "svk_damped")], dict(mode=1, stage2=True)),
    ("kbuf_mr_res2", KBUF, [case("res2", "mr")], dict(mode=1, stage2=True)),
    ("kbuf_wpb4_bunny", dict(KBUF, TLFEA_TANGENT_WPB="4"), [case("bunny", "svk")], dict(mode=1, stage2=True, wpb=4)),
    ("kbuf_wpb4_65", dict(KBUF, TLFEA_TANGENT_WPB="4"), [case("box_65", "mr")], dict(mode=1, stage2=True, wpb=4)),
    ("kbuf_pe_beam", KBUF, [case("beam_3x2x1", "table_svk"), case("beam_3x2x1", "table_mr")], dict(mode=1, stage2=True, wpb=1)),
    ("pe_star3_affine", {}, [case("star3", "table_svk")], dict(mode=3, lds_over_64k=True)),
    ("pe_star3_general", GENERAL, [case("star3", "table_svk")], dict(mode=2, lds_over_64k=True)),
    ("default_affine_bunny", {}, [case("bunny", "svk")], dict(mode=3)),
    ("default_general_bunny", GENERAL, [case("bunny", "svk")], dict(mode=2, rolled=1)),
    ("budgets_affine", {"TLFEA_AF_INST": "16", "TLFEA_AF_ACC": "256"}, [case("bunny", "svk")],
     dict(mode=3, more_groups_than="default_affine_bunny")),
    ("budgets_general", dict(GENERAL, TLFEA_AD_ACC="128"), [case("bunny", "svk")],
     dict(mode=2, more_groups_than="default_general_bunny")),
    ("few_waves_affine", {"TLFEA_AD_WAVES": "1"}, [case("res4", "svk_damped")], dict(mode=3, fewer_workgroups_than_groups=True)),
    ("few_waves_general", dict(GENERAL, TLFEA_AD_WAVES="1"), [case("res4", "svk_damped")],
     dict(mode=2, fewer_workgroups_than_groups=True)),
    ("mass_csr", {"TLFEA_MASS": "csr"}, [case("bunny", "svk_damped"), case("star3", "svk_damped")], dict(mode=3, gradient=1)),
    # a hub row of 155 KiB: neither fused form fits a workgroup's LDS (their staging comes on top), assemble_rows_kernel does
    # -- without a switch the set-up falls from the affine form to the general one to the two-kernel path
    ("falls_to_kbuf_cone", {}, [case("cone_22x20", "svk_damped")], dict(mode=1, stage2=True, lds_over_64k=True)),
    ("isolated_elem", {}, [case("isolated_box", "svk"), case("isolated_box", "mr")], dict()),
    ("isolated_elem_general", GENERAL, [case("isolated_box", "svk"), case("isolated_box", "mr")], dict(mode=2)),
    ("isolated_elem_kbuf", KBUF, [case("isolated_box", "svk"), case("isolated_box", "mr")], dict(mode=1, stage2=True)),
]
ISOLATED_MODES = {"svk": 3, "mr": 2}     # isolated_elem: what each material takes without a switch


# ---- inputs, shared by the worker and the judge -------------------------------------------------------------------------
def mesh_of(name):
    from tests import edge_meshes as em
    from tests.helpers import MESH_FILES, load_mesh
    if name in MESH_FILES:
        X, conn = load_mesh(name)
    else:
        X, conn = em.build(name)
    return np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(conn, dtype=np.int32)


def case_inputs(c):
    """everything both sides need: mesh, pinned nodes, state, loads, and for a material table the entry of every element"""
    from tests import edge_meshes as em
    from tests.helpers import MATERIALS, fixed_x0, perturbed_state
    X, conn = mesh_of(c["mesh"])
    fixed = fixed_x0(X)
    if "star" in c["mesh"] or "cone" in c["mesh"]:     # the hub sits at the origin: pinned only where the configuration says so
        hub = em.star_hub(X, conn)
        fixed = fixed[fixed != hub]
        if c.get("hub_pinned"):
            fixed = np.sort(np.append(fixed, hub)).astype(np.int32)
    if len(fixed) == 0:
        fixed = np.array([0, 3], dtype=np.int32)
    x, v = perturbed_state(X)
    rng = np.random.default_rng(7)
    f_ext = rng.normal(0, 1e3, 3 * X.shape[0])
    out = dict(X=X, conn=conn, fixed=np.ascontiguousarray(fixed, dtype=np.int32), x=x, v=v, vp=0.5 * v, f_ext=f_ext)
    if c["mat"].startswith("table_"):
        out["table"] = TABLES[c["mat"][6:]]
        cen = X[conn[:, :4]].mean(axis=1) - X.mean(axis=0)
        out["ids"] = ((cen[:, 0] > 0).astype(np.int32) + 2 * (cen[:, 1] > 0) + 4 * (cen[:, 2] > 0)).astype(np.int32) % 3   # by octant
        out["material"] = out["table"][0]
    else:
        out["material"] = MATERIALS[c["mat"]]
    return out


# ---- the judge (CPU only) -------------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0 and b.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def judge_hessian(n_nodes, ro, ci, val, ro_ref, ci_ref, val_ref, val_again=None, who=""):
    """H against the reference: index arrays bit-equal, values to TOL_ELEM of max|H|, the second assembly the same bits,
    symmetric to TOL_ELEM max|H| on meshes of at most 600 nodes.  Returns the relative error; raises AssertionError."""
    assert np.array_equal(ro, ro_ref) and np.array_equal(ci, ci_ref), (who, "index arrays differ from the oracle's")
    err = relerr(val, val_ref)
    assert err < TOL_ELEM, (who, "H", err)
    if val_again is not None:
        assert np.array_equal(val, val_again), (who, "the second assembly differs from the first")
    if n_nodes <= 600:
        import scipy.sparse as sp
        H = sp.csr_matrix((val, ci, ro), shape=(3 * n_nodes, 3 * n_nodes))
        asym = abs(H - H.T).max() if H.nnz else 0.0
        assert asym < TOL_ELEM * np.max(np.abs(val)), (who, "H is not symmetric", float(asym))
    return err


def oracle_reference(inp):
    """dict of the oracle's results on the inputs of case_inputs: det J, mass CSR, F, P, f_int, grad L, H.  One material:
    one oracle.  A material table: every quantity is a sum over elements, so one oracle per entry on that entry's elements
    (all N nodes kept; nodes without an element of the entry have empty rows there), summed; the constraint terms of grad L
    and H, which belong to nodes and not to elements, are added once, here."""
    import scipy.sparse as sp
    from tests.helpers import make_oracle
    X, conn, fixed, N = inp["X"], inp["conn"], inp["fixed"], inp["X"].shape[0]

    def run(m, sel, fx, f_ext):
        o = make_oracle(X, conn[sel], m, fx, f_ext)
        o.x, o.y, o.z = (np.ascontiguousarray(inp["x"][:, i]) for i in range(3))
        o.v, o.v_prev = inp["v"].copy(), inp["vp"].copy()
        F, P, _, _ = o.compute_p(None)
        f_int = o.internal_force(None)
        g = o.grad_L(o.internal_force(inp["v"]), H_STEP, RHO)
        ro, ci, val = o.assemble_hessian(H_STEP, RHO)
        return dict(o=o, detJ=o.detJ.copy(), F=F, P=P, f_int=f_int, g=g, ro=ro, ci=ci, val=val)

    everything = np.ones(conn.shape[0], dtype=bool)
    if "table" not in inp:
        r = run(inp["material"], everything, fixed, inp["f_ext"])
        o = r.pop("o")
        # F and P of the points in the engine's layout ([E, 5, 3, 3], row-major F)
        r["F"] = r["F"].reshape(-1, 5, 3, 3).transpose(0, 1, 3, 2)
        r["P"] = r["P"].reshape(-1, 5, 3, 3).transpose(0, 1, 3, 2)
        r.update(m_off=o.m_off, m_col=o.m_col, m_val=o.m_val)
        return r
    pattern = make_oracle(X, conn, inp["table"][0])            # index arrays of the whole mesh
    ro, ci = pattern.hessian_pattern()
    n = 3 * N
    Hsum, Msum = sp.csr_matrix((n, n)), sp.csr_matrix((N, N))
    out = dict(detJ=np.zeros((conn.shape[0], 5)), F=np.zeros((conn.shape[0], 5, 3, 3)), P=np.zeros((conn.shape[0], 5, 3, 3)),
               f_int=np.zeros(n), g=np.zeros(n))
    for k, m in enumerate(inp["table"]):
        sel = inp["ids"] == k
        assert sel.any(), "a table entry without elements"
        r = run(m, sel, None, None)
        out["detJ"][sel] = r["detJ"]
        out["F"][sel] = r["F"].reshape(-1, 5, 3, 3).transpose(0, 1, 3, 2)
        out["P"][sel] = r["P"].reshape(-1, 5, 3, 3).transpose(0, 1, 3, 2)
        out["f_int"] += r["f_int"]
        out["g"] += r["g"]                                     # M_k (v - v_prev) / h + f_int_k(x, v)
        Hsum = Hsum + sp.csr_matrix((r["val"], r["ci"], r["ro"]), shape=(n, n))
        o = r["o"]
        Msum = Msum + sp.csr_matrix((o.m_val, o.m_col, o.m_off), shape=(N, N))
    # node terms, once: - f_ext + h J^T (lam + rho c) with lam = 0, and h^2 rho on the pinned diagonal
    out["g"] -= inp["f_ext"]
    dofs = (3 * fixed[:, None] + np.arange(3)[None, :]).reshape(-1)
    c = (inp["x"] - X)[fixed].reshape(-1)
    out["g"][dofs] += H_STEP * RHO * c
    Hsum = Hsum + sp.csr_matrix((np.full(len(dofs), H_STEP * H_STEP * RHO), (dofs, dofs)), shape=(n, n))
    frame = sp.csr_matrix((np.zeros(len(ci)), ci, ro), shape=(n, n))     # the whole mesh's pattern, explicit zeros kept
    Hsum = (Hsum + frame).tocsr()
    Hsum.sort_indices()
    assert np.array_equal(Hsum.indptr, ro) and np.array_equal(Hsum.indices, ci), "the entries' patterns do not add up to the mesh's"
    mframe = sp.csr_matrix((np.zeros(len(pattern.m_col)), pattern.m_col, pattern.m_off), shape=(N, N))
    Msum = (Msum + mframe).tocsr()
    Msum.sort_indices()
    assert np.array_equal(Msum.indices, pattern.m_col)
    out.update(ro=ro, ci=ci, val=Hsum.data, m_off=pattern.m_off, m_col=pattern.m_col, m_val=Msum.data)
    return out


def judge_case(inp, ref, data, who=""):
    """every downloaded quantity of one case against the oracle's; returns the worst relative error of each"""
    N = inp["X"].shape[0]
    err = dict(detJ=relerr(data["detJ"], ref["detJ"]), mass=relerr(data["m_val"], ref["m_val"]), F=relerr(data["F"], ref["F"]),
               P=relerr(data["P"], ref["P"]), f_int=relerr(data["f_int"], ref["f_int"]), g=relerr(data["g"], ref["g"]))
    assert np.array_equal(data["m_off"], ref["m_off"]) and np.array_equal(data["m_col"], ref["m_col"]), (who, "mass pattern")
    assert err["detJ"] < TOL_GEOM and err["mass"] < TOL_GEOM, (who, err)
    for k in ("F", "P", "f_int", "g"):
        assert err[k] < TOL_ELEM, (who, k, err)
    err["H"] = judge_hessian(N, data["H_ro"], data["H_ci"], data["H_val"], ref["ro"], ref["ci"], ref["val"], data["H_val2"], who)
    return err


# ---- what every configuration must report -----------------------------------------------------------------------------------
def check_expect(name, expect, form, stages, c, gradient_form):
    """on the answers of tlfea_newton_get_assembly_form / _get_gradient_form and the stage counters of one assembly"""
    # 2: inertia rows from the residual launch + grad_light_kernel (the default); 1: mass CSR product in grad_kernel
    assert gradient_form == expect.get("gradient", 2), (name, gradient_form)
    mode = expect.get("mode", ISOLATED_MODES.get(c["mat"]))
    assert form["mode"] == mode, (name, c, form)
    if "rolled" in expect:
        assert form["rolled"] == expect["rolled"], (name, form)
    if "wpb" in expect:
        assert form["tangent_wpb"] == expect["wpb"], (name, form)
    if expect.get("lds_over_64k"):
        assert form["lds_bytes"] > 65536, (name, form)
    if expect.get("fewer_workgroups_than_groups"):
        assert form["workgroups"] < form["groups"], (name, form)
    # stage 2 (tangent blocks) runs exactly on the two-kernel path; the assembly stage always
    assert (stages["tangent_blocks"][1] > 0) == (form["mode"] == 1), (name, stages, form)
    assert stages["assemble_rows"][1] > 0, (name, stages)
    if form["mode"] != 1:
        assert form["groups"] >= 1 and form["passes"] >= form["groups"] and form["acc_max"] >= 9 * c["maxdeg"], (name, form)


# ---- the GPU side ---------------------------------------------------------------------------------------------------------
def run_case(c, tl):
    from tests.helpers import make_gpu
    inp = case_inputs(c)
    X, conn = inp["X"], inp["conn"]
    d = make_gpu(X, conn, inp["material"], inp["fixed"], inp["f_ext"])
    if "table" in inp:
        kind = inp["table"][0]["kind"]
        keys = ("E", "nu") if kind == "svk" else ("mu10", "mu01", "kappa")
        entries = [tl.ElementMaterial(rho0=m["rho0"], eta=m["eta"], lamd=m["lamd"], **{k: m[k] for k in keys}) for m in inp["table"]]
        d.SetElementMaterials(inp["ids"], entries, "svk" if kind == "svk" else "mooney_rivlin")
        d.CalcMassMatrix()
    out = dict(detJ=np.asarray(d.RetrieveDetJToCPU()))
    out["m_off"], out["m_col"], out["m_val"] = (np.asarray(a) for a in d.RetrieveMassCSRToCPU())
    x = inp["x"]
    d.UpdatePositions(x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy())
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-4, 1e-4, RHO, 5, 10, H_STEP))
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
    c = dict(c, maxdeg=int(np.diff(out["m_off"]).max()))
    del s
    d.Destroy()
    return c, form, stages, out, gform


def main(cfg, out_path):
    from tests.helpers import tl
    arrays, report = {}, []
    for k, c in enumerate(cfg["cases"]):
        c2, form, stages, out, gform = run_case(c, tl)
        check_expect(cfg["name"], cfg["expect"], form, stages, c2, gform)
        arrays.update({"c%d_%s" % (k, key): v for key, v in out.items()})
        report.append(dict(case=c, form=form, gradient_form=gform, stage_counts={key: v[1] for key, v in stages.items()}, N=int(len(out["m_off"]) - 1),
                           E=int(out["detJ"].shape[0])))
    np.savez(out_path, **arrays)
    print(json.dumps(dict(name=cfg["name"], cases=report)), flush=True)


if __name__ == "__main__":
    cfg = json.loads(sys.argv[1])
    for key, v in cfg["env"].items():
        assert os.environ.get(key) == v, "the caller did not set %s=%s" % (key, v)
    main(cfg, sys.argv[2])
