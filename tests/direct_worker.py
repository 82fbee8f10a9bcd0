"""Worker and configuration table of tests/test_gpu_direct_regimes.py: one configuration of the native sparse direct solve
(LinSolveOpts(method=1): csrc/mf_host.h plan, csrc/direct_kernels.hip) per process -- the library reads its TLFEA_DIRECT_*
switches once -- solving a handful of right-hand sides on the assembled H of a small mesh.

    python tests/direct_worker.py '<json config>' <out.npz>

config: name, problem, env (what the caller has put into the environment: the worker re-reads it to predict the
launches), mode ("solve", or the error paths "indefinite" / "refusal").  The worker asserts the regime: the plan facts the
device reports (tlfea_newton_get_direct_info / _fronts) are pushed through `plan_facts`, a restatement in Python of which
launches launch_mf_factor / launch_mf_solve issue for a plan and a set of switches; the launch tallies the library counted
must EQUAL that prediction, and the configuration's `expect` inequalities must hold on it.  A configuration that falls
back to the default path fails here.  It prints one JSON line and writes H, the right-hand sides, the solutions and the
info record to the npz; all judging arithmetic is the parent's, on the CPU.

The module is also imported by the CPU suite (tests/test_direct_plan.py), which evaluates the same `expect` inequalities
on the plan tests/native/mf_shim.cc builds for every configuration's mesh and switches, without a GPU."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NB = 48           # kMfNB: columns per panel step
WT = 128          # tile edge of mf_update_wide_kernel
NO_WIDE = {"TLFEA_DIRECT_WIDE_TILES": "1000000000"}   # pins the 64-tile trailing update: same tile kernel in every regime

# name, problem, environment.  What each must reach is in check_expect below.
CONFIGS = [
    ("default_res2", "res2", {}),
    ("default_bunny", "bunny", {}),
    ("natural_wide", "box_6_6_12", {}),
    ("one_front", "beam_3x2x1", {"TLFEA_DIRECT_LEAF": "256"}),
    ("deep_tree", "box_3_3_6", {"TLFEA_DIRECT_LEAF": "4"}),
    ("two_superpanels", "res4", {"TLFEA_DIRECT_LEAF": "256"}),
    ("super1", "res4", {"TLFEA_DIRECT_SUPER": "1"}),
    ("super2", "bunny", {"TLFEA_DIRECT_SUPER": "2"}),
    ("wide_forced", "res2", {"TLFEA_DIRECT_LEAF": "256", "TLFEA_DIRECT_WIDE_TILES": "1"}),
    ("wide_forced_super1", "bunny", {"TLFEA_DIRECT_SUPER": "1", "TLFEA_DIRECT_WIDE_TILES": "1"}),
    ("stepwise_all", "res2", {"TLFEA_DIRECT_ONE_WG_ROWS": "0"}),
    ("stepwise_all_leaf4", "bunny", {"TLFEA_DIRECT_LEAF": "4", "TLFEA_DIRECT_ONE_WG_ROWS": "0"}),
    ("stack_0", "res4", dict(NO_WIDE, TLFEA_DIRECT_TOP_DEPTH="0")),
    ("stack_2", "res4", dict(NO_WIDE, TLFEA_DIRECT_TOP_DEPTH="2")),
    ("stack_all", "res4", dict(NO_WIDE, TLFEA_DIRECT_TOP_DEPTH="99")),
    ("levels_ref", "res4", dict(NO_WIDE, TLFEA_DIRECT_TOP_DEPTH="-1")),
    ("stack_auto", "res4", {}),   # TLFEA_DIRECT_MAX_NNZ = L_total + floor(f F_total) of levels_ref: see stack_auto_env
    ("two_bodies_stack", "two_bodies", {"TLFEA_DIRECT_TOP_DEPTH": "0", "TLFEA_DIRECT_ONE_WG_ROWS": "0"}),
    ("ancf_plate", "plate3443", {"TLFEA_DIRECT_TOP_DEPTH": "0", "TLFEA_DIRECT_ONE_WG_ROWS": "0"}),
]
STACK_AUTO_FRACTIONS = (0.75, 0.5, 0.35)
ANCF = ("beam3243", "shell3443", "plate3443")


def stack_auto_env(levels_ref_info, f):
    """the memory bound (doubles) under which the plan has to leave whole-level workspaces by itself"""
    F_total = sum(levels_ref_info[k] for k in ("F_cap0", "F_cap1", "F_cap_work", "F_cap_stack"))
    return {"TLFEA_DIRECT_MAX_NNZ": str(levels_ref_info["L_total"] + int(f * F_total))}


# ---- meshes ------------------------------------------------------------------------------------------------------
def t10_mesh(problem):
    """(X, conn, fixed) of a T10 problem: the clamps of tests/test_gpu_direct.py"""
    from tests.helpers import fixed_x0, load_mesh, tl
    mu = tl.mesh_utils
    if problem.startswith("box_"):
        X, conn = mu.structured_t10_box(*(int(v) for v in problem.split("_")[1:]))
        fixed = np.where(X[:, 2] < 1e-12)[0].astype(np.int32)
    elif problem == "two_bodies":
        # two disconnected bodies of EQUAL node count: the median plane of the first cut then falls into the gap and the
        # root separator is empty.  (The 3x3x4 + 4x2x3 pair of test_direct_two_disconnected_bodies has 441 + 315 nodes: its
        # median lies inside the first body, the root gets a 189-column separator and the plan has no empty front at all.)
        Xa, ca = mu.structured_t10_box(3, 3, 4)
        Xb, cb = mu.structured_t10_box(3, 3, 4)
        X = np.vstack([Xa, Xb + np.array([5.0, 0.0, 0.0])])
        conn = np.vstack([ca, cb + Xa.shape[0]])
        fixed = np.where(X[:, 2] < 1e-12)[0].astype(np.int32)
    elif problem == "bunny":
        X, conn = load_mesh("bunny")
        fixed = np.where(X[:, 2] < X[:, 2].min() + 0.3)[0].astype(np.int32)
    else:
        X, conn = load_mesh(problem)
        fixed = fixed_x0(X)
    return X, np.ascontiguousarray(conn, dtype=np.int32), fixed


def plan_graph(problem):
    """(off, cols, x, y, z) the engine hands mf_plan_build for a problem: the node graph of H and the dissection coordinates
    (ANCF: a node's 4 coefficient vectors are 4 graph nodes at the node's position)"""
    from tests.test_rowgroups import adjacency
    if problem in ANCF:
        import tests.test_gpu_ancf as A
        _, x, y, z, conn = A.PROBLEMS[problem]()[:5]
        conn4 = (4 * np.asarray(conn, dtype=np.int64)[:, :, None] + np.arange(4)[None, None, :]).reshape(len(conn), -1)
        N = len(x)
        off, cols, _, _ = adjacency(conn4, N)
        X = np.stack([np.asarray(a, dtype=np.float64)[(np.arange(N) // 4) * 4] for a in (x, y, z)], axis=1)
    else:
        X, conn, _ = t10_mesh(problem)
        off, cols, _, _ = adjacency(conn, X.shape[0])
    return (np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32),
            *(np.ascontiguousarray(X[:, k]) for k in range(3)))


# ---- the launches of a plan, restated ----------------------------------------------------------------------------------
def switches(env):
    g = lambda k, d: int(float(env.get("TLFEA_DIRECT_" + k, d)))
    return dict(KS=NB * max(1, g("SUPER", 8)), wide_tiles=float(env.get("TLFEA_DIRECT_WIDE_TILES", 512)),
                one_wg_rows=g("ONE_WG_ROWS", 768))


def plan_facts(fronts, top_depth, env):
    """Plan facts and the launches launch_mf_factor / launch_mf_solve issue for the plan `fronts` ([n, 7]: c0, c1, depth,
    parent, node rows, child 0, child 1; children before parents) cut at `top_depth`, under the switches in `env`."""
    fr = np.asarray(fronts, dtype=np.int64).reshape(-1, 7)
    nf = len(fr)
    sw = switches(env)
    KS = sw["KS"]
    k, m, depth, parent = 3 * (fr[:, 1] - fr[:, 0]), 3 * fr[:, 4], fr[:, 2], fr[:, 3]
    child = fr[:, 5:7]
    maxd, T = int(depth.max()), int(top_depth)
    by_columns = lambda fl: sorted(fl, key=lambda f: (-k[f], f))
    # batches (mf_host.h): whole levels below the cut, the fronts of depth <= T one by one in postorder
    batches = []
    if T < 0:
        for d in range(maxd, -1, -1):
            batches.append((by_columns(np.where(depth == d)[0]), 0))
    else:
        anc = np.full(nf, -1)
        for f in range(nf - 1, -1, -1):
            anc[f] = -1 if depth[f] <= T else (parent[f] if depth[f] == T + 1 else anc[parent[f]])
        for f in range(nf):
            if depth[f] > T:
                continue
            if depth[f] == T:
                under = [g for g in range(f) if depth[g] > T and anc[g] == f]
                for d in range(maxd, T, -1):
                    fl = [g for g in under if depth[g] == d]
                    if fl:
                        batches.append((by_columns(fl), 0))
            batches.append(([f], 1 if parent[f] >= 0 else 0))
    t = dict(panel=0, update_inner=0, update_trailing=0, update_wide=0, extend_add=0, push=0, levels_one_wg=0,
             levels_stepwise=0, fwd_step=0, bwd_step=0)
    wide, trailing, max_below = [], [], 0   # per trailing launch: [(K, rows below the super-panel)] of its active fronts

    def steps_of(fl):
        out = []
        for j0 in range(0, int(k[fl[0]]) if len(fl) else 0, NB):
            act = [f for f in fl if k[f] > j0]
            out.append((j0, len(act), max(int(m[f] - j0 - min(NB, k[f] - j0)) for f in act)))
        return out

    for fl, push in batches:
        for slot in range(2):
            mu = max([int(m[c] - k[c]) for c in (child[f, slot] for f in fl) if c >= 0], default=0)
            t["extend_add"] += mu > 0
        steps = steps_of(fl)
        for i, (j0, na, mb) in enumerate(steps):
            S0 = (j0 // KS) * KS
            s1 = S0 + KS
            t["panel"] += 1
            max_below = max(max_below, mb)
            t["update_inner"] += mb > 0 and j0 + NB < s1
            if j0 + NB >= s1 or i + 1 == len(steps):
                act = fl[:steps[S0 // NB][1]]
                below = max(int(m[f] - min(s1, k[f])) for f in act)
                wt = (below + WT - 1) // WT
                if wt > 0:
                    big = wt * (wt + 1) / 2 * len(act) >= sw["wide_tiles"]
                    t["update_wide" if big else "update_trailing"] += 1
                    (wide if big else trailing).append([(int(min(s1, k[f]) - S0), int(m[f] - min(s1, k[f]))) for f in act])
        t["push"] += bool(push and m[fl[0]] > k[fl[0]])
    # the solve walks whole levels, deepest first
    stepwise = []     # per stepwise level: its fronts
    for d in range(maxd, -1, -1):
        fl = by_columns(np.where(depth == d)[0])
        if m[fl].max() <= sw["one_wg_rows"]:
            t["levels_one_wg"] += 1
            continue
        t["levels_stepwise"] += 1
        n_steps = len(steps_of(fl))
        t["fwd_step"] += n_steps
        t["bwd_step"] += n_steps
        stepwise.append(fl)
    t = {key: int(v) for key, v in t.items()}
    deepest = np.where(depth == maxd)[0]
    return dict(fronts=nf, levels=maxd + 1, top_depth=T, m_max=int(m.max()), k_max=int(k.max()), k_zero=int((k == 0).sum()),
                tally=t, wide=wide, trailing=trailing, max_below=int(max_below), k=k, m=m, depth=depth, parent=parent,
                stepwise=stepwise, deepest=deepest, KS=KS,
                nonempty_levels=int(sum(m[depth == d].max() > 0 for d in range(maxd + 1))),
                push_fronts=int(sum(depth[f] <= T and parent[f] >= 0 and m[f] > k[f] for f in range(nf))))


def check_expect(name, env, F):
    """the `expect` column of the configuration table, on the facts of plan_facts (or, on the GPU, on the facts AND the
    counted launches, which the worker has already required to be equal)"""
    t, k, m = F["tally"], F["k"], F["m"]
    all_sw = [f for fl in F["stepwise"] for f in fl]
    no_stack = F["top_depth"] == -1 and t["push"] == 0
    if name == "default_res2":          # no stack; every level one workgroup per front; 64-tiles only
        assert not env and no_stack and t["levels_stepwise"] == 0 and t["update_wide"] == 0 and t["update_trailing"] > 0, t
    elif name == "default_bunny":       # a stepwise level; a panel step with more than one 256-row block below it
        assert not env and t["levels_stepwise"] >= 1 and F["max_below"] > 256, (t, F["max_below"])
    elif name == "natural_wide":        # the default threshold is reachable without a switch
        assert not env and t["update_wide"] >= 1, t
    elif name == "one_front":           # one front, m = k = 315: last panel 27 columns wide, nothing below it
        assert F["fronts"] == 1 and F["m_max"] == F["k_max"] == 315 and 315 % NB == 27, (F["fronts"], F["m_max"], F["k_max"])
        assert t["panel"] == 7 and t["update_wide"] + t["update_trailing"] + t["extend_add"] == 0, t
    elif name == "deep_tree":           # > 100 fronts, >= 8 levels; the deepest level holds only fronts narrower than a panel
        assert F["fronts"] > 100 and F["levels"] >= 8, (F["fronts"], F["levels"])
        assert np.all((k[F["deepest"]] > 0) & (k[F["deepest"]] < NB)), k[F["deepest"]]
    elif name == "two_superpanels":     # a second, partial super-panel; a level that is stepwise by its size
        assert 384 < F["k_max"] < 768 and F["k_max"] % 384 != 0, F["k_max"]
        assert "TLFEA_DIRECT_ONE_WG_ROWS" not in env and t["levels_stepwise"] >= 1, t
    elif name == "super1":              # no update inside a super-panel; a trailing update after every panel with rows below
        assert F["KS"] == NB and t["update_inner"] == 0, t
        assert t["update_trailing"] + t["update_wide"] >= 1 and F["k_max"] > 2 * NB, (t, F["k_max"])
    elif name == "super2":              # both kinds of update
        assert F["KS"] == 2 * NB and t["update_inner"] > 0 and t["update_trailing"] + t["update_wide"] > 0, t
    elif name == "wide_forced":         # only 128-tiles; a trailing matrix that does not fill its last tile
        assert t["update_wide"] > 0 and t["update_trailing"] == 0, t
        assert any(below % WT != 0 for launch in F["wide"] for _, below in launch), F["wide"]
    elif name == "wide_forced_super1":  # 128-tiles with K = 48 and with a ragged K (its last chunk of 16 is masked)
        assert t["update_wide"] > 0 and t["update_trailing"] == 0 and t["update_inner"] == 0, t
        Ks = [K for launch in F["wide"] for K, below in launch if below > 0]
        assert NB in Ks and any(K % 16 != 0 for K in Ks), sorted(set(Ks))
    elif name == "stepwise_all":        # every level stepwise, panels narrower than 48 and grids of one block included
        assert t["levels_stepwise"] == F["nonempty_levels"] == F["levels"] and t["levels_one_wg"] == 0, t
        assert min(k[all_sw]) < NB and F["m_max"] <= 256, (min(k[all_sw]), F["m_max"])
    elif name == "stepwise_all_leaf4":  # as above, with fronts smaller than one panel (m < 48) and a front without own
        #                                 columns below the root in a stepwise level
        assert t["levels_stepwise"] == F["nonempty_levels"] and t["levels_stepwise"] >= F["levels"] - 1, t
        assert min(m[all_sw]) < NB and any(k[f] == 0 and F["parent"][f] >= 0 and m[f] > 0 for f in all_sw), (min(m[all_sw]), F["k_zero"])
    elif name in ("stack_0", "stack_2", "stack_all"):
        want = min(int(env["TLFEA_DIRECT_TOP_DEPTH"]), F["levels"] - 1)
        assert F["top_depth"] == want and (name != "stack_all" or want == F["levels"] - 1 < 99), (F["top_depth"], want)
        # pushes: the fronts of depth <= top_depth that have a parent (stack_0: the root alone is factored in the WORK buffer)
        assert t["push"] == F["push_fronts"] and (t["push"] > 0) == (want > 0) and t["update_wide"] == 0, (t, F["push_fronts"])
    elif name == "levels_ref":
        assert no_stack and t["update_wide"] == 0, (F["top_depth"], t)
    elif name == "stack_auto":          # the plan itself leaves whole-level workspaces
        assert "TLFEA_DIRECT_TOP_DEPTH" not in env and "TLFEA_DIRECT_MAX_NNZ" in env, env
        assert F["top_depth"] >= 0 and t["push"] == F["push_fronts"] > 0, (F["top_depth"], t)
    elif name == "two_bodies_stack":    # an empty root front in the stack regime, stepwise solves
        root = int(np.where(F["parent"] < 0)[0][0])
        assert F["top_depth"] == 0 and k[root] == 0 and m[root] == 0 and F["fronts"] > 1, (F["top_depth"], k[root], m[root])
        assert t["push"] == 0 and t["levels_stepwise"] == F["nonempty_levels"] == F["levels"] - 1, t
    elif name == "ancf_plate":          # coincident dissection coordinates: the 4 coefficient vectors of a node
        assert F["top_depth"] == 0 and t["levels_stepwise"] == F["nonempty_levels"] >= 2 and F["fronts"] > 1, (F["top_depth"], t)
    else:
        raise AssertionError("no expectation written for configuration %r" % name)
    # what no configuration may contain: a stepwise level none of whose fronts has a column (its launches would be empty)
    for fl in F["stepwise"]:
        assert k[fl].max() > 0, "a stepwise level without columns"


TALLY_KEYS = ("panel", "update_inner", "update_trailing", "update_wide", "extend_add", "push", "levels_one_wg",
              "levels_stepwise", "fwd_step", "bwd_step")


# ---- the GPU side ---------------------------------------------------------------------------------------------------------
def build(problem, material="neo", perturb=True, time_step=None):
    """(data, solver) with H ready to assemble: T10 as in tests/test_gpu_direct.py (positions moved by 1e-2 sin(pi X), so
    that the geometric stiffness is there), ANCF the randomly perturbed state of tests/precond_worker.py.  Time step 1e-3;
    1e-4 for ANCF: at 1e-3 the perturbed plate's H = M/h + h K has 15 negative eigenvalues (the CPU oracle's assembly of
    the same state, numpy eigvalsh; smallest -0.32), which a Cholesky factorisation rightly reports as not positive --
    at 1e-4 the smallest is +0.032 and cond(H) is 3e7."""
    if time_step is None:
        time_step = 1e-4 if problem in ANCF else 1e-3
    from tests.helpers import MATERIALS, make_gpu, tl
    if problem in ANCF:
        from tests.precond_worker import build_ancf
        d, s = build_ancf(problem)[:2]
    else:
        X, conn, fixed = t10_mesh(problem)
        d = make_gpu(X, conn, MATERIALS[material], fixed)
        if perturb:
            x = X + 1e-2 * np.sin(np.pi * X)
            d.UpdatePositions(x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy())
        s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-6, 1e-4, 1e14, 5, 10, time_step))
    return d, s


def hessian(s):
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    return dict(H_ro=np.asarray(ro), H_ci=np.asarray(ci), H_val=np.asarray(val))


def own_dofs(order, front):
    nodes = order[front[0]:front[1]]
    return (3 * nodes[:, None] + np.arange(3)[None, :]).reshape(-1)


def solve_mode(cfg, out_path):
    from tests.helpers import tl
    d, s = build(cfg["problem"])
    s.AssembleHessian()
    data = hessian(s)
    n = len(data["H_ro"]) - 1
    # on_unconverged=1: the library's own residual guard (1e-8, measured with its own SpMV) does not stand between a
    # wrong solution and the parent's judgement on the CPU, whose bounds are seven orders tighter
    s.SetLinSolveOpts(tl.LinSolveOpts(method=1, on_unconverged=1))
    b_rand = np.random.default_rng(3).normal(size=n)
    sols, rels, its = {}, {}, {}

    def solve(tag, b):
        x, it, rel = s.LinearSolve(b)
        sols[tag], its[tag], rels[tag] = np.array(x), int(it), float(rel)

    solve("b_rand", b_rand)                      # builds the plan
    info = s.GetDirectInfo()
    order, fronts = s.GetDirectFronts()
    facts = plan_facts(fronts, info["top_depth"], cfg["env"])
    # ---- the regime this configuration is named for ------------------------------------------------------------
    for key in ("fronts", "levels", "m_max", "k_max", "k_zero"):
        assert facts[key] == info[key], (cfg["name"], key, facts[key], info[key])
    counted = {key: info[key] for key in TALLY_KEYS}
    assert counted == facts["tally"], "%s: launches counted %r, predicted from the plan %r" % (cfg["name"], counted, facts["tally"])
    check_expect(cfg["name"], cfg["env"], facts)
    # ---- right-hand sides ------------------------------------------------------------------------------------------------
    k, depth = facts["k"], facts["depth"]
    leaf = int(np.where((depth == depth.max()) & (k > 0))[0][0])          # a deepest front
    root = int(np.where(k > 0)[0][-1])                                     # the last non-empty front of the elimination
    rng = np.random.default_rng(17)
    B = {"b_rand": b_rand, "b_ones": np.ones(n), "b_leaf": np.zeros(n), "b_root": np.zeros(n), "b_zero": np.zeros(n)}
    for tag, f in (("b_leaf", leaf), ("b_root", root)):
        idx = own_dofs(order, fronts[f])
        B[tag][idx] = rng.normal(size=idx.size)
    for tag in ("b_ones", "b_leaf", "b_root", "b_zero"):
        solve(tag, B[tag])
    x1 = sols["b_rand"]
    solve("b_rand", b_rand)
    info2 = s.GetDirectInfo()
    assert {key: info2[key] for key in TALLY_KEYS} == counted, (info2, counted)    # the counters restart with every solve
    tags = list(B)
    keys = list(tl.SyncedNewtonSolver.DIRECT_INFO_KEYS)
    data.update(B=np.array([B[t] for t in tags]), X=np.array([sols[t] for t in tags]), X_first=x1, tags=np.array(tags),
                rel=np.array([rels[t] for t in tags]), it=np.array([its[t] for t in tags]),
                info=np.array([info[key] for key in keys], dtype=np.int64), info_keys=np.array(keys), order=order, fronts=fronts)
    np.savez(out_path, **data)
    print(json.dumps(dict(name=cfg["name"], n=int(n), info=info, leaf_front=leaf, root_front=root, max_below=facts["max_below"])),
          flush=True)
    del s
    d.Destroy()


def indefinite_mode(cfg, out_path):
    """A pivot that is not positive under a forced regime is reported, and the same solver object then solves a definite H:
    the error flag and the workspaces are reset by the next factorisation."""
    from tests.helpers import tl
    d, s = build(cfg["problem"], material="svk", perturb=False, time_step=-1e-3)   # H = M/h + hK with h < 0: indefinite
    s.AssembleHessian()
    s.SetLinSolveOpts(tl.LinSolveOpts(method=1))
    n = 3 * s.n_coef
    b = np.random.default_rng(3).normal(size=n)
    try:
        s.LinearSolve(b)
        message = ""
    except RuntimeError as e:
        message = str(e)
    assert s.GetDirectInfo()["top_depth"] == 0, s.GetDirectInfo()
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-6, 1e-4, 1e14, 5, 10, 1e-3))
    s.AssembleHessian()
    data = hessian(s)
    x, it, rel = s.LinearSolve(b)
    info = s.GetDirectInfo()
    assert info["F_cap_work"] > 0 and info["update_inner"] == 0 and info["update_trailing"] > 0, info   # the forced regime
    data.update(B=b[None, :], X=np.array(x)[None, :], rel=np.array([rel]), it=np.array([it]))
    np.savez(out_path, **data)
    print(json.dumps(dict(name=cfg["name"], message=message, info=info)), flush=True)
    del s
    d.Destroy()


def refusal_mode(cfg, out_path):
    """A plan that does not fit its memory bound is refused with a message; the solver object still solves iteratively."""
    from tests.helpers import tl
    d, s = build(cfg["problem"])
    s.AssembleHessian()
    data = hessian(s)
    n = len(data["H_ro"]) - 1
    b = np.random.default_rng(3).normal(size=n)
    s.SetLinSolveOpts(tl.LinSolveOpts(method=1))
    try:
        s.LinearSolve(b)
        message = ""
    except RuntimeError as e:
        message = str(e)
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-12, 20000, 10))
    x, it, rel = s.LinearSolve(b)
    data.update(B=b[None, :], X=np.array(x)[None, :], rel=np.array([rel]), it=np.array([it]))
    np.savez(out_path, **data)
    print(json.dumps(dict(name=cfg["name"], message=message, it=int(it), rel=float(rel))), flush=True)
    del s
    d.Destroy()


if __name__ == "__main__":
    cfg = json.loads(sys.argv[1])
    for key, v in cfg["env"].items():
        assert os.environ.get(key) == v, "the caller did not set %s=%s" % (key, v)
    {"solve": solve_mode, "indefinite": indefinite_mode, "refusal": refusal_mode}[cfg.get("mode", "solve")](cfg, sys.argv[2])
