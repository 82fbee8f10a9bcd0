"""Worker of tests/test_gpu_precond_operator.py: one configuration of the CG preconditioner compared, as an operator,
with its fp64 restatement (tests/precond_np.py).  The library reads its TLFEA_* switches once per process, so every
configuration runs in its own process (the caller sets the environment).

    python tests/precond_worker.py '<json config>' <out.npz>

config: problem (a T10 mesh tag, or beam3243 / shell3443 / plate3443), opts [cheb_degree, cheb_kappa, cheb_bits, precond],
expect (the preconditions of the path this configuration pins; the worker FAILS when one does not hold).  Prints one JSON
line with the measured figures and writes what the parent needs to rebuild the restatement (for the fp32 floor, which is
computed in the parent on the CPU) to the npz."""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import precond_np as pn  # noqa: E402
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_gpu, tl  # noqa: E402

OMEGA = np.array([0.3, -0.5, 0.8])


def lanes_rule(n_rows, n_blocks):
    """lanes per row the polynomial step picks from the mean blocks per row ("Linear solve"), unless TLFEA_C32_LANES forces it"""
    forced = int(os.environ.get("TLFEA_C32_LANES", "0"))
    if forced in (8, 16, 32):
        return forced
    avg = n_blocks / max(1, n_rows)
    return 32 if avg > 48.0 else (8 if avg <= 18.0 else 16)


def build_t10(tag):
    return build_t10_mesh(*load_mesh(tag))


def build_t10_mesh(X, conn):
    fixed = fixed_x0(X)
    d = make_gpu(X, conn, MATERIALS["svk"], fixed)
    x = X + np.random.default_rng(7).normal(0.0, 1e-4, X.shape)
    x[fixed] = X[fixed]
    d.UpdatePositions(x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy())
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    c = X.mean(axis=0)
    trans = np.tile([1.0, 0.0, 0.0], X.shape[0])
    rot = np.cross(OMEGA, X - c).reshape(-1)
    return d, s, fixed, trans, rot


def build_ancf(name):
    import tests.test_gpu_ancf as A
    prob = A.PROBLEMS[name]()
    o, d = A.make_pair(prob, A.SVK)
    fixed = np.asarray(prob[6], dtype=np.int64)
    rng = np.random.default_rng(5)
    ref = [np.array(a, dtype=np.float64) for a in (o.xt, o.yt, o.zt)]
    xs = [a + rng.normal(0, 1e-3, a.shape) for a in ref]
    for a, r in zip(xs, ref):
        a[fixed] = r[fixed]
    d.UpdatePositions(*xs)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    # rigid motions of an ANCF mesh: position coefficients (slot 0 of a node's four) move as points, gradients as vectors
    C = np.stack(ref, axis=1)
    pos = np.arange(C.shape[0]) % 4 == 0
    trans = np.where(pos[:, None], np.array([1.0, 0.0, 0.0])[None, :], 0.0).reshape(-1)
    rot = np.where(pos[:, None], np.cross(OMEGA, C - C[pos].mean(axis=0)), np.cross(OMEGA, C)).reshape(-1)
    return d, s, fixed, trans, rot


def relnorm(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main(cfg, out_path):
    ancf = cfg["problem"] in ("beam3243", "shell3443", "plate3443")
    d, s, fixed, trans, rot = (build_ancf if ancf else build_t10)(cfg["problem"])
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-4, 1e-4, 1e14, 5, 10, 1e-3))
    deg, kappa, bits, pre = cfg["opts"]
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 20000, 1, deg, kappa, bits, pre))
    s.AssembleHessian()
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    n = len(ro) - 1
    N = n // 3
    H = sp.csr_matrix((val, ci, ro), shape=(n, n))
    blocks = np.diff(ro)[::3] // 3                                   # 3 x 3 blocks per node row
    out = dict(name=cfg["name"], N=int(N), blocks_min=int(blocks.min()), blocks_max=int(blocks.max()),
               blocks_mean=float(blocks.mean()))

    # ---- vectors ----------------------------------------------------------------------------------------------
    rng = np.random.default_rng(11)
    names, vecs = [], []
    for k in range(3):
        names.append("normal%d" % k); vecs.append(rng.normal(size=n))
    i_max, i_min = int(np.argmax(blocks)), int(np.argmin(blocks))
    for tag, node in (("impulse_longest_row", i_max), ("impulse_shortest_row", i_min)):
        for c in range(3):
            e = np.zeros(n); e[3 * node + c] = 1.0
            names.append("%s_%s" % (tag, "xyz"[c])); vecs.append(e)
    names += ["rigid_translation", "rigid_rotation"]; vecs += [trans, rot]
    if len(fixed):
        v = np.zeros(n)
        idx = (3 * np.asarray(fixed, dtype=np.int64)[:, None] + np.arange(3)[None, :]).reshape(-1)
        v[idx] = rng.normal(size=len(idx))
        names.append("pinned_only"); vecs.append(v)
    R = np.array(vecs)

    # ---- the device's operator: one set-up (from normal0), every vector --------------------------------------------
    Z = s.ApplyPreconditioner(R)
    state = s.GetPreconditionerState()
    info = dict(linsolve=s.GetLinSolveInfo(), poly=s.GetPolynomialInfo(), cycle=s.GetPmgCycleInfo(), precond=s.GetPreconditioner())
    store = int(info["linsolve"][1])
    out.update(store=store, precond=state["precond"], levels=state["levels"], degree=state["degree"], ks=state["ks"],
               ks2=state["ks2"], kc=state["kc"], k3=state["k3"], block=state["block"], smoother=state["smoother"],
               lam=list(state["hook_lam"]), lam_safety=state["lam_safety"], lanes_fine=lanes_rule(N, int(blocks.sum())))
    data = dict(R=R, **pn.pack_device_state(s, H, store, state, out))
    if state["precond"] == 2:
        out["lanes_vertex"] = lanes_rule(out["n_vertex"], out["vertex_blocks"])

    # ---- preconditions of the path this configuration pins -----------------------------------------------------------
    ex = cfg.get("expect", {})
    checks = {"precond": out["precond"], "levels": out["levels"], "degree": out["degree"], "store": store, "ks": out["ks"],
              "block": out["block"], "lanes_fine": out["lanes_fine"], "lanes_vertex": out.get("lanes_vertex"),
              "smoother": out["smoother"]}
    for key, want in ex.items():
        if key in checks:
            assert checks[key] == want, "%s: %s is %r, the configuration needs %r" % (cfg["name"], key, checks[key], want)
    if "blocks_max_gt" in ex:
        assert out["blocks_max"] > ex["blocks_max_gt"], (cfg["name"], "longest row", out["blocks_max"])
    if "blocks_min_lt" in ex:
        assert out["blocks_min"] < ex["blocks_min_lt"], (cfg["name"], "shortest row", out["blocks_min"])
    if "vertex_blocks_max_gt" in ex:
        assert out["vertex_blocks_max"] > ex["vertex_blocks_max_gt"], (cfg["name"], "vertex rows", out["vertex_blocks_max"])
    if ex.get("identity_rows"):  # switched-off rotations or empty aggregates: identity rows of H3
        assert out["inactive_rotations"] + out["empty_cells"] >= 1, (cfg["name"], out["inactive_rotations"], out["empty_cells"])
    if ex.get("two_rows"):
        # 256-thread groups of two rows: the last group of a level must run without a second row
        assert int(os.environ.get("TLFEA_C32_BW_N", "-1")) == 0
        assert N % (2 * (256 // out["lanes_fine"])) != 0, (N, out["lanes_fine"])
        if state["precond"] == 2:
            assert out["n_vertex"] % (2 * (256 // out["lanes_vertex"])) != 0, (out["n_vertex"], out["lanes_vertex"])

    # ---- (a) operator match, (c) positivity -----------------------------------------------------------------------------
    op = pn.operator_from(data, state)
    Zref = np.array([op(r) for r in R])
    out["finite"] = bool(np.all(np.isfinite(Z)))
    out["err"] = {nm: relnorm(z, zr) for nm, z, zr in zip(names, Z, Zref)}
    out["xMx"] = {nm: float(r @ z) / float(np.linalg.norm(r) * np.linalg.norm(z)) for nm, r, z in zip(names, R, Z)}
    # ---- (b) symmetry on two pairs of the normal vectors ------------------------------------------------------------------
    out["sym"] = [float(abs(R[a] @ Z[b] - R[b] @ Z[a]) / (np.linalg.norm(R[a]) * np.linalg.norm(Z[b]))) for a, b in ((0, 1), (1, 2))]
    # ---- (d) determinism, independence of earlier calls, the zero vector ----------------------------------------------------
    z1, z2 = s.ApplyPreconditioner(R[0]), s.ApplyPreconditioner(R[0])
    out["bitwise_repeat"] = bool(np.array_equal(z1, z2))
    out["bitwise_block_vs_single"] = bool(np.array_equal(z1, Z[0]))
    z0 = s.ApplyPreconditioner(np.zeros(n))
    out["zero_exact"] = bool(np.all(z0 == 0.0))
    # ---- (e) the path CG itself takes ------------------------------------------------------------------------------------------
    b = np.random.default_rng(3).normal(size=n)
    x_gpu, its_gpu, rel = s.LinearSolve(b)
    st_e = s.GetPreconditionerState()
    op_e = pn.operator_from(data, st_e)
    x_np, its_np, rel_np = pn.pcg(H, b, op_e, 1e-12)
    out.update(its_gpu=int(its_gpu), its_np=int(its_np), rel_gpu=float(rel), rel_np=float(rel_np),
               x_relerr=float(np.abs(x_gpu - x_np).max() / np.abs(x_np).max()), lam_safety_solve=st_e["lam_safety"])
    data.update(b=b, names=np.array(names), coef=state["coef"], coef_solve=st_e["coef"],
                layout=pn.layout_of(state), layout_solve=pn.layout_of(st_e), layout_keys=np.array(pn.LAYOUT_KEYS))
    np.savez(out_path, **data)
    print(json.dumps(out), flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    main(json.loads(sys.argv[1]), sys.argv[2])
