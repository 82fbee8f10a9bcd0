"""Per-element materials on the GPU (tlfea_t10_set_element_materials): a one-entry table against the uniform path, a
mixed table against the unchanged oracle by linearity, an analytic series bar, disjoint bodies in one object against
one object per body, determinism, stiffness contrast and the refusals."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import (MATERIALS, csr_to_dense, fixed_x0, load_mesh, make_gpu, make_oracle, perturbed_state,
                           relerr)

tl = importlib.import_module("total-lagrangian-fea_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")


def entry(m):
    """ElementMaterial of a helpers.MATERIALS record."""
    keys = ("E", "nu") if m["kind"] == "svk" else ("mu10", "mu01", "kappa")
    return tl.ElementMaterial(rho0=m["rho0"], eta=m["eta"], lamd=m["lamd"], **{k: m[k] for k in keys})


def model(m):
    return "svk" if m["kind"] == "svk" else "mooney_rivlin"


def set_table(d, ids, mats, mdl):
    """A table on an object made by make_gpu: the mass matrix is assembled again with the table's densities."""
    d.SetElementMaterials(ids, mats, mdl)
    d.CalcMassMatrix()


def hessian(d, h=1e-3, rho=1e12, env=None, monkeypatch=None):
    if monkeypatch is not None:
        if env:
            monkeypatch.setenv("TLFEA_ASSEMBLE", env)
        else:
            monkeypatch.delenv("TLFEA_ASSEMBLE", raising=False)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-4, 1e-4, rho, 5, 10, h))
    s.AnalyzeHessianSparsity()
    mode = s.GetAssemblyMode()
    s.AssembleHessian()
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    del s
    return mode, ro, ci, val


def state(d):
    d.CalcP()
    d.CalcInternalForce()
    return dict(F=d.RetrieveDeformationGradientToCPU(), P=d.RetrievePFromFToCPU(), f=d.RetrieveInternalForceToCPU(),
                M=d.RetrieveMassCSRToCPU()[2])


def fixed_of(X):
    f = fixed_x0(X)
    return f if len(f) else np.array([0, 3], dtype=np.int32)


# ---- 1. one-entry table == uniform path ----------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["beam_3x2x1", "bunny"])
@pytest.mark.parametrize("mat", ["svk", "svk_damped", "mr_damped"])
@pytest.mark.parametrize("form", [None, "general"])
def test_one_entry_table_equals_uniform(tag, mat, form, monkeypatch):
    X, conn = load_mesh(tag)
    m = MATERIALS[mat]
    fixed = fixed_of(X)
    x, _ = perturbed_state(X)
    out = []
    for table in (False, True):
        d = make_gpu(X, conn, m, fixed)
        if table:
            set_table(d, np.zeros(conn.shape[0], dtype=np.int32), [entry(m)], model(m))
            assert np.array_equal(d.GetElementMaterialIds(), np.zeros(conn.shape[0]))
        d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])
        st = state(d)
        mode, _, _, st["H"] = hessian(d, env=form, monkeypatch=monkeypatch)
        if m["kind"] == "svk":
            assert mode == (2 if form else 3)
        # one Newton step with damping (velocity guess from the perturbed state)
        s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
        s.SetParameters(tl.SyncedNewtonParams(0.0, 0.0, 0.0, 1e12, 1, 2, 1e-3))
        s.SetLinSolveOpts(tl.LinSolveOpts(1e-13, 20000, 10))
        s.Solve()
        st["x"] = np.stack(d.RetrievePositionToCPU(), axis=1)
        del s
        d.Destroy()
        out.append(st)
    u, t = out
    for k in ("F", "P", "f", "M", "H"):
        assert relerr(t[k], u[k]) <= 1e-13, k
    assert np.max(np.abs(t["x"] - u["x"])) <= 1e-13 * np.max(np.abs(u["x"])) + 1e-12 * np.max(np.abs(u["x"] - x))


# ---- 2. mixed table against the oracle by linearity ---------------------------------------------------------------
def _oracle_part(X, conn, sel, m, fixed, x):
    o = make_oracle(X, conn[sel], m, fixed)
    o.x, o.y, o.z = (np.ascontiguousarray(x[:, i]) for i in range(3))
    return o


@pytest.mark.parametrize("tag", ["beam_3x2x1", "cube"])
@pytest.mark.parametrize("kind", ["svk", "mr"])
def test_mixed_table_linearity(tag, kind):
    X, conn = load_mesh(tag)
    E, N = conn.shape[0], X.shape[0]
    if kind == "svk":
        mA = dict(kind="svk", E=7e8, nu=0.33, rho0=2700.0, eta=1e5, lamd=2e5)
        mB = dict(kind="svk", E=3e7, nu=0.45, rho0=900.0, eta=3e3, lamd=0.0)
    else:
        mA = dict(kind="mr", mu10=4e7, mu01=1e7, kappa=5e8, rho0=920.0, eta=2e4, lamd=3e4)
        mB = dict(kind="mr", mu10=2e6, mu01=5e5, kappa=4e7, rho0=1500.0, eta=0.0, lamd=1e3)
    zero = dict(mA, rho0=0.0, eta=0.0, lamd=0.0, **({"E": 0.0} if kind == "svk" else dict(mu10=0.0, mu01=0.0, kappa=0.0)))
    ids = (np.arange(E) % 3 == 1).astype(np.int32)    # B: every third element
    A, B = ids == 0, ids == 1
    fixed = fixed_of(X)
    x, _ = perturbed_state(X)
    h, rho = 1e-3, 1e12
    d = make_gpu(X, conn, mA, fixed)
    set_table(d, ids, [entry(mA), entry(mB)], model(mA))
    d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])
    st = state(d)
    _, ro, ci, val = hessian(d, h, rho)
    Hg = csr_to_dense(ro, ci, val, 3 * N)
    mo, mc, mv = d.RetrieveMassCSRToCPU()
    Mg = csr_to_dense(mo, mc, mv, N)
    d.Destroy()
    oA, oB = _oracle_part(X, conn, A, mA, fixed, x), _oracle_part(X, conn, B, mB, fixed, x)
    o0, oA0, oB0 = (_oracle_part(X, conn, sel, zero, fixed, x) for sel in (np.ones(E, bool), A, B))
    f_ref = oA.internal_force() + oB.internal_force()
    assert relerr(st["f"], f_ref) <= 1e-12
    M_ref = csr_to_dense(oA.m_off, oA.m_col, oA.m_val, N) + csr_to_dense(oB.m_off, oB.m_col, oB.m_val, N)
    assert relerr(Mg, M_ref) <= 1e-12
    # H_A + H_B - H_0, where each part's own constraint terms (its zero-material H) are taken out first: a pinned node
    # outside a part's elements has no row in that part's pattern
    H = [csr_to_dense(*o.assemble_hessian(h, rho), 3 * N) for o in (oA, oB, o0, oA0, oB0)]
    assert relerr(Hg, (H[0] - H[3]) + (H[1] - H[4]) + H[2]) <= 1e-12


# ---- 3. analytic series bar ---------------------------------------------------------------------------------------
def series_bar():
    """2 x 1 x 1 box, x in [0, 2], split at x = 1 on element faces; SVK nu = 0, E1 = 1e7, E2 = 1e8; the axial stretch
    lam_i per half makes P11 = E_i (lam_i^2 - 1)/2 lam_i equal in both halves."""
    X, conn = tl.mesh_utils.structured_t10_box(4, 2, 2, 2.0, 1.0, 1.0)
    cx = X[conn[:, :4]].mean(axis=1)[:, 0]
    ids = (cx > 1.0).astype(np.int32)
    E1, E2 = 1e7, 1e8
    lam1 = 1.01
    p = E1 * (lam1 ** 2 - 1) / 2 * lam1
    # E2 (l^2 - 1) l / 2 = p  ->  Newton on l
    lam2 = 1.0
    for _ in range(60):
        g = E2 * (lam2 ** 3 - lam2) / 2 - p
        lam2 -= g / (E2 * (3 * lam2 ** 2 - 1) / 2)
    x = X.copy()
    x[:, 0] = np.where(X[:, 0] <= 1.0, lam1 * X[:, 0], lam1 + lam2 * (X[:, 0] - 1.0))
    return X, conn, ids, x, (E1, E2)


def test_series_bar_interior_equilibrium():
    X, conn, ids, x, (E1, E2) = series_bar()
    d = make_gpu(X, conn, MATERIALS["svk"])
    d.SetElementMaterials(ids, [tl.ElementMaterial(E=E1, nu=0.0, rho0=1000.0), tl.ElementMaterial(E=E2, nu=0.0, rho0=1000.0)])
    d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])
    f = state(d)["f"].reshape(-1, 3)
    d.Destroy()
    left, right = np.abs(X[:, 0]) < 1e-12, np.abs(X[:, 0] - 2.0) < 1e-12
    inner = ~(left | right)
    F_end = np.linalg.norm(f[right].sum(axis=0))
    assert F_end > 0
    assert np.max(np.abs(f[inner])) <= 1e-10 * F_end
    assert np.max(np.abs(f[left].sum(axis=0) + f[right].sum(axis=0))) <= 1e-10 * F_end
    # the host driver prints the same numbers
    exe = os.path.join(HOST, "test_two_material_bar")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST, "test_two_material_bar"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout
    vals = dict(line.split("=", 1) for line in out.split() if "=" in line)
    assert float(vals["interior_max"]) <= 1e-10 * float(vals["end_force"])
    assert abs(float(vals["end_force"]) - F_end) <= 1e-9 * F_end


# ---- 4. disjoint bodies: one object against one object per body ---------------------------------------------------
def _two_bodies():
    X, conn = load_mesh("beam_3x2x1")
    shift = np.array([0.0, 5.0, 0.0])
    X2 = np.vstack([X, X + shift])
    conn2 = np.vstack([conn, conn + X.shape[0]])
    return X, conn, X2, conn2


def _run(d, n_con, solver, method):
    if solver == "newton":
        s = tl.SyncedNewtonSolver(d, n_con)
        s.SetParameters(tl.SyncedNewtonParams(0.0, 0.0, 0.0, 1e12, 1, 3, 1e-3))
        s.SetLinSolveOpts(tl.LinSolveOpts(1e-14, 20000, 10, method=method, on_unconverged=1))
    elif solver == "adamw":
        s = tl.SyncedAdamWNocoopSolver(d, n_con)
        s.SetParameters(tl.SyncedAdamWNocoopParams(lr=1e-4, inner_tol=0.0, outer_tol=0.0, rho=1e12, max_outer=1,
                                                   max_inner=30))
    elif solver == "nesterov":
        s = tl.SyncedNesterovSolver(d, n_con)
        s.SetParameters(tl.SyncedNesterovParams(alpha=1e-9, rho=1e12, inner_tol=0.0, outer_tol=0.0, max_outer=1,
                                                max_inner=30))
    else:
        s = tl.SyncedVBDSolver(d, n_con)
        s.SetParameters(tl.SyncedVBDParams(inner_tol=0.0, inner_rtol=0.0, outer_tol=0.0, rho=1e12, max_outer=1,
                                           max_inner=10))
    s.Solve()
    x = np.stack(d.RetrievePositionToCPU(), axis=1)
    del s
    return x


@pytest.mark.parametrize("solver,method,tol", [("newton", 0, 1e-10), ("newton", 1, 1e-12), ("adamw", 0, 1e-10),
                                               ("nesterov", 0, 1e-10), ("vbd", 0, 1e-10)])
def test_disjoint_bodies(solver, method, tol):
    X, conn, X2, conn2 = _two_bodies()
    mA = dict(kind="svk", E=7e8, nu=0.33, rho0=2700.0, eta=1e4, lamd=1e4)
    mB = dict(kind="svk", E=5e7, nu=0.4, rho0=1200.0, eta=0.0, lamd=2e3)
    n = X.shape[0]
    fx = fixed_x0(X)
    f1 = np.zeros(3 * n)
    f1[3 * np.where(np.abs(X[:, 0] - X[:, 0].max()) < 1e-9)[0] + 2] = -2e4
    xs = []
    for m in ((mA, mB) if solver not in ("adamw", "vbd") else ()):
        d = make_gpu(X, conn, m, fx, f1)
        xs.append(_run(d, d.get_n_constraint(), solver, method))
        d.Destroy()
    fx2, f2 = np.concatenate([fx, fx + n]), np.concatenate([f1, f1])
    if solver in ("adamw", "vbd"):
        # these steps couple the bodies through global quantities (AdamW's norms, the colouring of VBD's sweep), so
        # one object of two bodies is compared with the same object on the uniform path: a table of two equal entries
        xs = []
        for table in (False, True):
            d = make_gpu(X2, conn2, mA, fx2, f2)
            if table:
                set_table(d, np.repeat([0, 1], conn.shape[0]).astype(np.int32), [entry(mA), entry(mA)], "svk")
            xs.append(_run(d, d.get_n_constraint(), solver, method))
            d.Destroy()
        disp = np.max(np.abs(xs[0] - X2))
        assert disp > 0
        assert np.max(np.abs(xs[1] - xs[0])) <= tol * disp + 8 * np.finfo(float).eps * np.max(np.abs(X2))
        return
    d = make_gpu(X2, conn2, mA, fx2, f2)
    set_table(d, np.repeat([0, 1], conn.shape[0]).astype(np.int32), [entry(mA), entry(mB)], "svk")
    x2 = _run(d, d.get_n_constraint(), solver, method)
    d.Destroy()
    for k in range(2):
        xb = x2[k * n:(k + 1) * n] - (k * np.array([0.0, 5.0, 0.0]))
        xr = xs[k]
        disp = np.max(np.abs(xr - X))
        assert disp > 0
        assert np.max(np.abs(xb - xr)) <= tol * disp + 8 * np.finfo(float).eps * np.max(np.abs(X2)), (solver, k)


# ---- 5. determinism -------------------------------------------------------------------------------------------------
def test_determinism():
    X, conn = load_mesh("bunny")
    m = MATERIALS["svk_damped"]
    ids = (np.arange(conn.shape[0]) % 2).astype(np.int32)
    x, _ = perturbed_state(X)
    res = []
    for _ in range(2):
        d = make_gpu(X, conn, m, fixed_of(X))
        set_table(d, ids, [entry(m), tl.ElementMaterial(E=1e7, nu=0.2, rho0=500.0, eta=10.0)], "svk")
        d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])
        f = state(d)["f"]
        res.append((f, hessian(d)[3]))
        d.Destroy()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- 6. stiffness contrast ----------------------------------------------------------------------------------------
def test_stiffness_contrast(capsys):
    X, conn = tl.mesh_utils.structured_t10_box(12, 12, 12)
    cz = X[conn[:, :4]].mean(axis=1)[:, 2]
    ids = (cz > 0.5).astype(np.int32)
    fixed = np.where(np.abs(X[:, 2]) < 1e-12)[0].astype(np.int32)
    f = np.zeros(3 * X.shape[0])
    top = np.where(np.abs(X[:, 2] - 1.0) < 1e-12)[0]
    f[3 * top + 2] = -2000.0 / len(top)
    iters = {}
    for c in (1, 10, 100, 1000):
        d = make_gpu(X, conn, MATERIALS["svk"], fixed, f)
        set_table(d, ids, [tl.ElementMaterial(E=7e8, nu=0.33, rho0=2700.0),
                           tl.ElementMaterial(E=7e8 / c, nu=0.33, rho0=2700.0)], "svk")
        ok = True
        for method in (0, 1):
            s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
            s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-6, 1e-4, 1e14, 1, 2, 1e-3))
            s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 20000, 10, method=method, on_unconverged=1))
            s.Solve()
            st = s.GetLinSolveStatus()
            if method == 0:
                iters[c] = (s.GetStats()["pcg_iters"], st["worst_rel_res"])
                ok = st["all_converged"]
                del s
                if ok:
                    break
            else:
                assert st["all_converged"], (c, st)   # the direct solve takes the step the CG missed
                del s
        if c < 1000:
            assert ok, (c, iters[c])
        d.Destroy()
    with capsys.disabled():
        print(f"\nstiffness contrast -> (CG iterations, worst rel residual): {iters}")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def _err(lib):
    return lib.tlfea_last_error().decode()


def test_refusals():
    lib = tl.load_library()
    X, conn = load_mesh("beam_3x2x1")
    E = conn.shape[0]
    d = make_gpu(X, conn, MATERIALS["svk"], fixed_x0(X))
    tab = (tl.binding.MaterialEntryC * 2)(tl.binding.MaterialEntryC(7e8, 0.3, 0, 0, 0, 1000, 0, 0),
                                          tl.binding.MaterialEntryC(7e7, 0.3, 0, 0, 0, 1000, 0, 0))
    ids = np.zeros(E, dtype=np.int32)
    ip = tl.binding.ip
    ids[3] = 2
    assert lib.tlfea_t10_set_element_materials(d._h, 0, 2, tab, ip(ids), E) != 0
    assert "outside 0..1" in _err(lib)
    ids[3] = 1
    assert lib.tlfea_t10_set_element_materials(d._h, 0, 2, tab, ip(ids), E - 1) != 0
    assert "n_elem" in _err(lib)
    bad = (tl.binding.MaterialEntryC * 1)(tl.binding.MaterialEntryC(7e8, 0.5, 0, 0, 0, 1000, 0, 0))
    assert lib.tlfea_t10_set_element_materials(d._h, 0, 1, bad, ip(ids * 0), E) != 0
    assert "nu must be in (-1, 0.5)" in _err(lib)
    assert lib.tlfea_t10_set_element_materials(d._h, 2, 2, tab, ip(ids), E) != 0
    assert "unknown model" in _err(lib)
    assert lib.tlfea_t10_set_element_materials(d._h, 0, 257, tab, ip(ids), E) != 0
    assert "n_mat" in _err(lib)
    assert lib.tlfea_t10_set_element_materials(d._h, 0, 2, tab, ip(ids), E) == 0
    for call in (lambda: d.SetSVK(1e8, 0.3), lambda: d.SetMooneyRivlin(1, 1, 1), lambda: d.SetDensity(1.0),
                 lambda: d.SetDamping(1.0, 1.0)):
        with pytest.raises(tl.TlfeaError, match="per-element materials are set"):
            call()
    # the partitioned path refuses before any collective is touched: minimal one-rank lists, callbacks never called
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    sh = s._h
    called = []
    ar = tl.binding.ALLREDUCE_FN(lambda *a: called.append(1) or 1)
    ex = tl.binding.HALO_EXCHANGE_FN(lambda *a: called.append(1) or 1)
    N = X.shape[0]
    layer = np.zeros(N, dtype=np.int32)
    z1 = np.zeros(1, dtype=np.int32)
    lists = tl.binding.HaloListsC(0, ip(z1), ip(z1), ip(z1), ip(z1), ip(z1), ip(z1), 0, 1)
    lib.tlfea_newton_set_halo.argtypes = None
    assert lib.tlfea_newton_set_halo(sh, ip(layer), 3, C.byref(lists), ar, ex, None, 0) != 0
    assert "per-element materials" in _err(lib)
    nodes = np.arange(N, dtype=np.int32)
    w = np.ones(N)
    assert lib.tlfea_newton_set_interface(sh, ip(nodes), ip(nodes), N, N, tl.binding.dp(w), ar, None, 0) != 0
    assert "per-element materials" in _err(lib)
    assert not called
    del s
    d.ClearElementMaterials()
    assert d.GetElementMaterialIds() is None
    d.SetSVK(1e8, 0.3)    # uniform again
    d.Destroy()
    # an ANCF handle
    a = tl.GPU_ANCF3243_Data(2, 1)
    a.Initialize()
    assert lib.tlfea_t10_set_element_materials(a._h, 0, 1, tab, ip(np.zeros(1, dtype=np.int32)), 1) != 0
    assert "ANCF" in _err(lib)
    a.Destroy()
