"""Worker of tests/test_gpu_cg_trace.py: one configuration of the CG iteration traced for k iterations through
SyncedNewtonSolver.CGTrace and checked step by step with tests/cg_np.py.  The library reads its TLFEA_* switches once per
process, so every configuration runs in its own process (the caller sets the environment).

    python tests/cg_trace_worker.py '<json config>' <out.npz>

config: problem (res2 | plate3443 | box), opts [cheb_degree, cheb_kappa, cheb_bits, precond], k, expect (the form the
hook must report; the worker FAILS when it reports another), classes (the row classes the mesh must have), z_records.
Prints one JSON line with the worst ratio of every measured error to its bound and writes the iterates the parent
compares across configurations to the npz."""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cg_np  # noqa: E402
from tests import precond_np as pn  # noqa: E402
from tests import precond_worker as pw  # noqa: E402
from tests.helpers import tl  # noqa: E402

BOX = (20, 20, 19)   # 41 x 41 x 39 = 65 559 node rows: the smallest box over the 65 536 rows of the XCD-eighth sweep


def build(problem):
    if problem == "box":
        return pw.build_t10_mesh(*tl.mesh_utils.structured_t10_box(*BOX))[:2]
    return (pw.build_ancf if problem == "plate3443" else pw.build_t10)(problem)[:2]


def traced(cfg, b=None):
    d, s = build(cfg["problem"])
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-4, 1e-4, 1e14, 5, 10, 1e-3))
    deg, kappa, bits, pre = cfg["opts"]
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 20000, 1, deg, kappa, bits, pre))
    s.AssembleHessian()
    if b is None:
        b = np.random.default_rng(3).normal(size=3 * s.n_coef)
    return d, s, b, s.CGTrace(b, cfg["k"])


def main(cfg, out_path):
    d, s, b, tr = traced(cfg)
    f = tr["form"]
    k, n = cfg["k"], b.size
    N = n // 3
    out = dict(name=cfg["name"], N=int(N), form=f)

    # ---- the form this configuration pins -------------------------------------------------------------------------
    for key, want in cfg["expect"].items():
        assert f[key] == want, "%s: the hook reports %s = %r, the configuration needs %r (%r)" % (cfg["name"], key, f[key], want, f)
    if cfg["problem"] == "box":
        assert N >= 65536 and f["grid"] == 512, (N, f["grid"])
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    H = sp.csr_matrix((val, ci, ro), shape=(n, n))
    classes = cg_np.row_classes(H, f["lanes"])
    out["row_classes"] = classes
    for c in cfg["classes"]:
        assert classes[c] > 0, "%s: no node row of class %d at %d lanes %r" % (cfg["name"], c, f["lanes"], classes)

    # ---- the restated preconditioner (polynomial forms) -----------------------------------------------------------------
    precond, z_bound = None, None
    if f["update"] != 0:
        state = s.GetPreconditionerState()
        store = int(s.GetLinSolveInfo()[1])
        data = pn.pack_device_state(s, H, store, state, out)
        precond, op32 = pn.operator_from(data, state, np.float64), pn.operator_from(data, state, np.float32)
        nz = min(k, cfg.get("z_records") or k)
        floor = max(float(np.linalg.norm(op32(r) - precond(r)) / np.linalg.norm(precond(r))) for r in tr["r"][:nz])
        z_bound = 1e-10 if store == 64 else min(8.0 * floor, 1e-3)
        out.update(store=store, floor=floor, z_bound=z_bound, precond=state["precond"], block=state["block"])
        assert state["precond"] == f["precond"] and (state["block"] == 12) == bool(f["block12"]), (state["precond"], state["block"], f)
    try:
        out["ratios"] = cg_np.check_trace(H, b, tr, precond, z_bound, cfg.get("z_records"))
    except cg_np.TraceError as e:
        out["failed"] = str(e)

    # ---- the same configuration again, from a fresh solver: bit for bit ------------------------------------------------------
    del s
    d.Destroy()
    d2, s2, _, tr2 = traced(cfg, b)
    differ = {}
    for key in ("x", "r", "z", "p", "q", "sums", "slots"):
        ne = (tr[key] != tr2[key]).reshape(k + 1, -1)
        if ne.any():  # first record that differs, how many of its entries, the first of them
            j = int(np.argmax(ne.any(axis=1)))
            differ[key] = [j, int(ne[j].sum()), int(np.argmax(ne[j]))]
    out["repeat_differs"] = differ
    out["bitwise_repeat"] = not differ and tr["form"] == tr2["form"]
    del s2
    d2.Destroy()

    small = n <= 30000
    keep = {key: (tr[key] if small else tr[key][:2]) for key in ("x", "r", "z", "p", "q")}
    np.savez(out_path, sums=tr["sums"], **keep)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(json.loads(sys.argv[1]), sys.argv[2])
