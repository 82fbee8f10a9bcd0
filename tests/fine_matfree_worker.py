"""Worker of tests/test_gpu_fine_matfree.py.  The library reads its TLFEA_* switches once per process, so every scenario runs
as `python -m tests.fine_matfree_worker '<json config>' <out.npz>` in a fresh child (the caller sets the environment).
Prints one JSON line last.

config: what = "operator" | "solve", mesh (tests/galerkin_np.py: beam_3x2x1, box, permuted), material (a tests/helpers.py
tag, or [E, time step] for St.Venant-Kirchhoff with Kelvin-Voigt damping), variant = "" | "per_element" | "obstacle".

    operator  ApplyPreconditioner against the restatement tests/fine_matfree_np.py, one pass in each of its three coefficient
              forms against the fp64 CSR evaluation of the same formula, R against S_c P^T H S_f, one solve
    solve     one LinearSolve from a seeded right-hand side: iterations, residuals, read-backs; x goes to the npz"""
import json
import sys

import numpy as np
import scipy.sparse as sp

from tests import fine_matfree_np as fm
from tests import galerkin_np as gn
from tests import precond_np as pn
from tests import restricted_op_np as rn
from tests.helpers import MATERIALS, fixed_x0, make_gpu, tl


def build(cfg):
    X, conn = gn.mesh(cfg["mesh"])
    mat, h = cfg.get("material", "svk_damped"), 1e-3
    if not isinstance(mat, str):
        E, h = mat
        m = dict(MATERIALS["svk_damped"], E=E, eta=1e-4 * E * h, lamd=1e-4 * E * h)
    else:
        m = MATERIALS[mat]
    fixed = fixed_x0(X)
    assert len(fixed) > 0
    d = make_gpu(X, conn, m, fixed)
    if cfg.get("variant") == "per_element":
        mats = [tl.ElementMaterial(**{k: v for k, v in dict(m, E=m["E"] * f).items() if k != "kind"}) for f in (1.0, 2.0)]
        d.SetElementMaterials((np.arange(conn.shape[0]) % 2).astype(np.int32), mats, model="svk")
    if cfg.get("variant") == "obstacle":
        d.SetRigidObstacles([tl.RigidPlane((0.0, 0.0, -1e-3), (0.0, 0.0, 1.0), 1e8)])
    x = X + np.random.default_rng(7).normal(0.0, 1e-4, X.shape)
    x[fixed] = X[fixed]
    d.UpdatePositions(x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy())
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(1e-8, 0.0, 1e-8, 1e14, 2, 4, h))
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 20000, 1))
    s.EvalGradient()
    s.AssembleHessian()
    q = tl.quadrature
    ep = fm.element_problem(X, conn, x, (q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights), m["E"], m["nu"], m["rho0"], h,
                            m["eta"], m["lamd"], fixed, 1e14)
    return X, conn, d, s, fixed, ep


def relnorm(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def inf_dist(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def single_passes(s, H, state, out, data):
    """one pass in each coefficient form -- a Chebyshev pair, the restart pair (0, 1/theta), the last pass -- from the same
    float32 start vectors, twice, against the step of the fp64 CSR level evaluated in float64 on those vectors"""
    L = fm.fine_level(H)
    n = H.shape[0]
    rng = np.random.default_rng(21)
    r = rng.normal(size=n)
    coef = np.asarray(state["coef"], dtype=np.float64)
    res = (L.sc * r).astype(np.float32)
    d = (L.dinv(res.astype(np.float64)) * coef[0] + 0.1 * coef[0] * rng.normal(size=n)).astype(np.float32)
    z = (d.astype(np.float64) * (1.0 + 0.5 * rng.normal(size=n))).astype(np.float32)
    # (c1, c2, weight of the z^ update, last); the weight of the first form is not 1, so that it shows
    forms = {"chebyshev": (coef[2], coef[3], 1.25, False), "restart": (0.0, coef[state["cf_restart"] + 1], 1.0, False),
             "last": (coef[2], coef[3], 1.0, True)}
    d64, z64, res64 = (a.astype(np.float64) for a in (d, z, res))
    out["pass"] = {}
    for nm, (c1, c2, w, last) in forms.items():
        a = s.FineSmootherPass(d, res, z, r, [c1, c2], 0.0 if w == 1.0 else w, last)
        b = s.FineSmootherPass(d, res, z, r, [c1, c2], 0.0 if w == 1.0 else w, last)
        o = dict(bitwise=bool(all(np.array_equal(u, v) for u, v in zip(a, b))), finite=bool(all(np.all(np.isfinite(u)) for u in a)))
        if last:
            dr, zr, rz = fm.last_pass(L, d64, z64, res64, r, c1, c2, w)
            o.update(d=inf_dist(a[0], dr), z=inf_dist(a[1], zr), rz_ref_rel=abs(float(a[2].sum()) - rz) / abs(rz),
                     slots_rel=abs(float(a[2].sum()) - float(r @ a[1])) / abs(float(r @ a[1])),
                     slots_used=int(np.count_nonzero(a[2])))
        else:
            dr, zr, rr = L.step(d64, z64, res64, c1, c2, w)
            o.update(d=inf_dist(a[0], dr), z=inf_dist(a[1], zr), res=inf_dist(a[2], rr))
        out["pass"][nm] = o
    data.update(pass_d=d, pass_z=z, pass_res=res, pass_r=r, pass_names=np.array(list(forms)),
                pass_coef=np.array([[v[0], v[1], v[2], float(v[3])] for v in forms.values()]))


def solve(s, H, out):
    n = H.shape[0]
    b = np.random.default_rng(3).normal(size=n)
    x, its, rel = s.LinearSolve(b)
    out.update(its_gpu=int(its), rel_gpu=float(rel), true_res=float(np.linalg.norm(b - H @ x) / np.linalg.norm(b)),
               finite=bool(np.all(np.isfinite(x))), fine_smoother_solve=s.GetFineSmoother(), spmv_mode=s.GetSpmvMode())
    return b, x


def main(cfg, out_path):
    X, conn, d, s, fixed, ep = build(cfg)
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    n = len(ro) - 1
    H = sp.csr_matrix((val, ci, ro), shape=(n, n))
    out = dict(what=cfg["what"], mesh=cfg["mesh"], N=n // 3, E=int(conn.shape[0]), assembly=s.GetAssemblyMode())
    if cfg["what"] == "solve":
        b, x = solve(s, H, out)
        np.savez(out_path, x=x, b=b, **pn.pack_csr("H", H))
        print(json.dumps(out), flush=True)
        del s
        d.Destroy()
        return

    rng = np.random.default_rng(11)
    names = ["normal0", "normal1", "normal2"]
    vecs = [rng.normal(size=n) for _ in range(3)]
    blocks = np.diff(ro)[::3] // 3
    for tag, node in (("impulse_longest_row", int(np.argmax(blocks))), ("impulse_shortest_row", int(np.argmin(blocks)))):
        e = np.zeros(n); e[3 * node + 1] = 1.0
        names.append(tag); vecs.append(e)
    v = np.zeros(n)
    idx = (3 * np.asarray(fixed, dtype=np.int64)[:, None] + np.arange(3)[None, :]).reshape(-1)
    v[idx] = rng.normal(size=len(idx))
    names.append("pinned_only"); vecs.append(v)
    R = np.array(vecs)

    Z = s.ApplyPreconditioner(R)
    out["fine_smoother"] = s.GetFineSmoother()
    state = s.GetPreconditionerState()
    out.update(precond=state["precond"], levels=state["levels"], ks=state["ks"], smoother=state["smoother"])
    data = dict(R=R, **ep, **pn.pack_device_state(s, H, 16, state, out))
    single_passes(s, H, state, out, data)
    op = fm.element_operator_from(data, state)
    Zref = np.array([op(r) for r in R])
    out["finite_z"] = bool(np.all(np.isfinite(Z)))
    out["err"] = {nm: relnorm(z, zr) for nm, z, zr in zip(names, Z, Zref)}
    out["xMx"] = {nm: float(r @ z) / float(np.linalg.norm(r) * np.linalg.norm(z)) for nm, r, z in zip(names, R, Z)}
    out["sym"] = [float(abs(R[a] @ Z[b] - R[b] @ Z[a]) / (np.linalg.norm(R[a]) * np.linalg.norm(Z[b]))) for a, b in ((0, 1), (1, 2))]
    z1, z2 = s.ApplyPreconditioner(R[0]), s.ApplyPreconditioner(R[0])
    out["bitwise_repeat"] = bool(np.array_equal(z1, z2) and np.array_equal(z1, Z[0]))
    out["zero_exact"] = bool(np.all(s.ApplyPreconditioner(np.zeros(n)) == 0.0))

    # R = S_c P^T H S_f, block by block in fp64, against the device's float32 R; two builds
    info = s.GetRestrictOpInfo()
    out["rop_active"] = info["active"]
    if info["active"] == 1:
        off, cols, vals = s.RetrieveRestrictOp()
        f_off, f_cols, _, sc_f, sc_c = s.RetrieveFineCopy()
        par0, par1 = s.RetrievePmgLevel()[:2]
        s.ApplyPreconditioner(R[0])
        off2, cols2, vals2 = s.RetrieveRestrictOp()
        out["r_bitwise_rebuild"] = bool(np.array_equal(off, off2) and np.array_equal(cols, cols2) and np.array_equal(vals, vals2))
        r_off, r_cols, r_vals, r_mag = rn.restricted_operator_blocks(f_off, f_cols, fm.scaled_blocks(H, f_off, f_cols, sc_f), sc_f,
                                                                     sc_c, par0, par1)
        out["r_pattern_equal"] = bool(np.array_equal(off, r_off) and np.array_equal(cols, r_cols))
        if out["r_pattern_equal"]:
            out["r_worst_excess"] = float((np.abs(vals - r_vals) - 2.0 ** -23 * r_mag).max())
            out["r_worst_rel"] = float((np.abs(vals - r_vals) / np.maximum(r_mag, 1e-300)).max())

    b, x_gpu = solve(s, H, out)
    st_e = s.GetPreconditionerState()
    x_np, its_np, rel_np = pn.pcg(H, b, fm.element_operator_from(data, st_e), 1e-12)
    out.update(its_np=int(its_np), rel_np=float(rel_np), x_relerr=float(np.abs(x_gpu - x_np).max() / np.abs(x_np).max()))
    data.update(b=b, names=np.array(names), coef=state["coef"], coef_solve=st_e["coef"], layout=pn.layout_of(state),
                layout_solve=pn.layout_of(st_e), layout_keys=np.array(pn.LAYOUT_KEYS))
    np.savez(out_path, **data)
    print(json.dumps(out), flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    main(json.loads(sys.argv[1]), sys.argv[2])
