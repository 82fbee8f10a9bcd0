"""Host plan of the engine's own sparse direct solve (csrc/mf_host.h): nested-dissection fronts, row structures, extend-add
maps, H -> front entry lists and level order, checked end to end by EXECUTING the plan with plain loops on the CPU
(tests/native/mf_shim.cc) against scipy's sparse solve.  Integer work + a dense reference executor -- runs without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.helpers import load_mesh
from tests.test_rowgroups import adjacency, dp, ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mu = __import__("importlib").import_module("total-lagrangian-fea_amd.mesh_utils")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("mf") / "libmf_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "mf_shim.cc")])
    lib = C.CDLL(str(so))
    lib.mf_build.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                             C.POINTER(C.c_double), C.c_int, C.c_longlong, C.POINTER(C.c_longlong)]
    return lib


def spd_in_engine_layout(N, off, cols, seed):
    """random SPD matrix on the node pattern, in the engine's value layout (node row i: 9 off[i] + d * 3 deg + 3 k + e)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(N), np.diff(off))
    blk = rng.normal(size=(cols.size, 3, 3))
    key = {(int(r), int(c)): t for t, (r, c) in enumerate(zip(rows, cols))}
    for t, (r, c) in enumerate(zip(rows, cols)):
        if c < r:
            blk[t] = blk[key[(int(c), int(r))]].T
        elif c == r:
            blk[t] = 0.5 * (blk[t] + blk[t].T) + 9.0 * (off[r + 1] - off[r]) * np.eye(3)
    vals = np.zeros(9 * cols.size)
    ri, ci, vv = [], [], []
    for t, (r, c) in enumerate(zip(rows, cols)):
        deg = off[r + 1] - off[r]
        k = t - off[r]
        for d in range(3):
            base = 9 * off[r] + d * 3 * deg + 3 * k
            vals[base:base + 3] = blk[t][d]
            for e in range(3):
                ri.append(3 * r + d)
                ci.append(3 * c + e)
                vv.append(blk[t][d, e])
    return vals, sp.csc_matrix((vv, (ri, ci)), shape=(3 * N, 3 * N))


@pytest.mark.parametrize("mesh,leaf", [("box", 8), ("box", 32), ("res2", 16), ("bunny", 32), ("beam_3x2x1", 4)])
def test_plan_factors_and_solves(shim, mesh, leaf):
    if mesh == "box":
        X, conn = mu.structured_t10_box(4, 3, 3, 2.0, 1.5, 1.5)
    else:
        X, conn = load_mesh(mesh)
    conn = np.ascontiguousarray(conn, dtype=np.int32)
    N = X.shape[0]
    off, cols, _, _ = adjacency(conn, N)
    x, y, z = (np.ascontiguousarray(X[:, k]) for k in range(3))
    info = (C.c_longlong * 8)()
    assert shim.mf_build(N, ip(off), ip(cols), dp(x), dp(y), dp(z), leaf, 1 << 40, info) == 0
    nf, nl = int(info[0]), int(info[1])
    order = np.zeros(N, dtype=np.int32)
    c0, c1, par, dep, nr = (np.zeros(nf, dtype=np.int32) for _ in range(5))
    shim.mf_fetch(ip(order), ip(c0), ip(c1), ip(par), ip(dep), ip(nr))
    assert np.array_equal(np.sort(order), np.arange(N))                       # a permutation
    own = np.zeros(N, dtype=np.int32)
    for f in range(nf):
        own[c0[f]:c1[f]] += 1
        assert par[f] == -1 or (par[f] > f and dep[par[f]] == dep[f] - 1 and c0[par[f]] >= c1[f])
        assert nr[f] >= c1[f] - c0[f]
    assert np.all(own == 1) and (par == -1).sum() == 1 and dep.max() + 1 == nl   # every node owned once, one root
    assert int(info[7]) == (cols.size + N) // 2                                 # one entry per lower node block
    vals, A = spd_in_engine_layout(N, off, cols, 5)
    b = np.random.default_rng(7).normal(size=3 * N)
    xo = np.zeros(3 * N)
    assert shim.mf_cpu_factor_solve(dp(vals), dp(b), dp(xo)) == 0
    ref = spla.spsolve(A, b)
    assert np.linalg.norm(xo - ref) <= 1e-12 * np.linalg.norm(ref)
    assert np.linalg.norm(A @ xo - b) <= 1e-13 * np.linalg.norm(b)
    # a memory bound that the whole-level workspaces exceed: the tree is cut into subtrees that reuse their workspaces
    # (what lets config C's 118 GB factor fit next to its fronts); same ordering, same factor, same solution
    L, ws = int(info[2]), int(info[3]) + int(info[4])
    info2 = (C.c_longlong * 8)()
    for frac in (0.75, 0.5, 0.35):
        if shim.mf_build(N, ip(off), ip(cols), dp(x), dp(y), dp(z), leaf, L + int(frac * ws), info2) != 0:
            continue
        assert int(info2[2]) == L and int(info2[3]) + int(info2[4]) <= frac * ws and int(info2[4]) > 0
        x2 = np.zeros(3 * N)
        assert shim.mf_cpu_factor_solve(dp(vals), dp(b), dp(x2)) == 0
        assert np.linalg.norm(x2 - xo) <= 1e-13 * np.linalg.norm(xo)


def _regime_plan(shim, graph, env, monkeypatch):
    """the plan the engine builds for a graph under the TLFEA_DIRECT_* switches in env: (fronts [n, 7], top_depth, info) or None"""
    off, cols, x, y, z = graph
    monkeypatch.delenv("TLFEA_DIRECT_TOP_DEPTH", raising=False)
    if "TLFEA_DIRECT_TOP_DEPTH" in env:                     # read by mf_plan_build itself, per plan
        monkeypatch.setenv("TLFEA_DIRECT_TOP_DEPTH", env["TLFEA_DIRECT_TOP_DEPTH"])
    info = (C.c_longlong * 8)()
    leaf, bound = int(env.get("TLFEA_DIRECT_LEAF", 32)), int(env.get("TLFEA_DIRECT_MAX_NNZ", 1 << 40))
    if shim.mf_build(len(x), ip(off), ip(cols), dp(x), dp(y), dp(z), leaf, bound, info) != 0:
        return None
    assert shim.mf_check_bounds() == 0      # what the kernels will address lies inside the buffers the plan sizes
    fronts, reg = np.zeros(7 * int(info[0]), dtype=np.int32), (C.c_longlong * 5)()
    shim.mf_fronts(ip(fronts))
    shim.mf_regime(reg)
    return fronts.reshape(-1, 7), int(reg[0]), dict(L_total=int(info[2]), F_cap0=int(reg[1]), F_cap1=int(reg[2]),
                                                    F_cap_work=int(reg[3]), F_cap_stack=int(reg[4]))


def test_regime_configurations_reach_their_regimes(shim, monkeypatch):
    """Every configuration of tests/test_gpu_direct_regimes.py (table and `expect` inequalities: tests/direct_worker.py),
    evaluated on the plan this host builds for its mesh and switches: a mesh or a switch that stops reaching the kernel
    regime it is there for is caught here, without a GPU.  The launches are those plan_facts predicts; on the GPU the
    worker requires the launches the library counted to equal that prediction."""
    from tests import direct_worker as dw
    graphs, facts, spd = {}, {}, {}
    for name, problem, env in dw.CONFIGS:
        if problem not in graphs:
            graphs[problem] = dw.plan_graph(problem)
        assert 3 * len(graphs[problem][2]) <= 13000, (problem, "the matrix is to stay a small mesh")
        if name == "stack_auto":
            continue
        fronts, top, info = _regime_plan(shim, graphs[problem], env, monkeypatch)
        facts[name] = dict(dw.plan_facts(fronts, top, env), **info)
        dw.check_expect(name, env, facts[name])
        if name in ("stack_0", "stack_2", "stack_all", "levels_ref", "two_bodies_stack"):
            # the forced cuts, executed: WORK buffer, stack pushes and pops give the solution of the whole-level plan
            if problem not in spd:
                N = len(graphs[problem][2])
                vals, A = spd_in_engine_layout(N, graphs[problem][0], graphs[problem][1], 5)
                b = np.random.default_rng(7).normal(size=3 * N)
                spd[problem] = (vals, b, spla.spsolve(A, b))
            vals, b, ref = spd[problem]
            xo = np.zeros_like(b)
            assert shim.mf_cpu_factor_solve(dp(vals), dp(b), dp(xo)) == 0
            assert np.linalg.norm(xo - ref) <= 1e-12 * np.linalg.norm(ref), name
    # the plan's own choice of the stack regime: the first memory bound of the list that it accepts
    problem = dict((c[0], c[1]) for c in dw.CONFIGS)["stack_auto"]
    for f in dw.STACK_AUTO_FRACTIONS:
        env = dw.stack_auto_env(facts["levels_ref"], f)
        got = _regime_plan(shim, graphs[problem], env, monkeypatch)
        if got is not None:
            dw.check_expect("stack_auto", env, dw.plan_facts(got[0], got[1], env))
            break
    else:
        raise AssertionError("the plan accepts none of the memory bounds of stack_auto")
    # the four configurations that are compared bit by bit share the ordering and the fronts
    for name in ("stack_0", "stack_2", "stack_all"):
        assert all(np.array_equal(facts[name][key], facts["levels_ref"][key]) for key in ("k", "m", "depth", "parent"))
        assert facts[name]["L_total"] == facts["levels_ref"]["L_total"]


def test_plan_refuses_what_does_not_fit(shim):
    X, conn = mu.structured_t10_box(4, 3, 3, 2.0, 1.5, 1.5)
    conn = np.ascontiguousarray(conn, dtype=np.int32)
    N = X.shape[0]
    off, cols, _, _ = adjacency(conn, N)
    x, y, z = (np.ascontiguousarray(X[:, k]) for k in range(3))
    info = (C.c_longlong * 8)()
    assert shim.mf_build(N, ip(off), ip(cols), dp(x), dp(y), dp(z), 16, 1000, info) == 1


def _solve_on_graph(shim, N, pairs, leaf, seed=1):
    """SPD matrix on an arbitrary node graph (pairs of adjacent nodes), planned, factored and solved on the CPU"""
    adj = [set([i]) for i in range(N)]
    for a, b in pairs:
        adj[a].add(b)
        adj[b].add(a)
    off = np.zeros(N + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(a) for a in adj])
    cols = np.concatenate([np.array(sorted(a), dtype=np.int32) for a in adj])
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, 3))
    x, y, z = (np.ascontiguousarray(X[:, k]) for k in range(3))
    info = (C.c_longlong * 8)()
    assert shim.mf_build(N, ip(off), ip(cols), dp(x), dp(y), dp(z), leaf, 1 << 40, info) == 0
    vals, A = spd_in_engine_layout(N, off, cols, seed)
    b = rng.normal(size=3 * N)
    xo = np.zeros(3 * N)
    assert shim.mf_cpu_factor_solve(dp(vals), dp(b), dp(xo)) == 0
    assert np.linalg.norm(A @ xo - b) <= 1e-12 * np.linalg.norm(b)
    return int(info[0]), int(info[1])


def test_plan_edge_cases(shim):
    """One node; a mesh smaller than a leaf (one front); a chain (every separator is one node); two disconnected components
    (an empty separator at the root: a front without own columns); a complete graph (one dense front after all)."""
    assert _solve_on_graph(shim, 1, [], 4) == (1, 1)
    assert _solve_on_graph(shim, 7, [(i, i + 1) for i in range(6)], 32) == (1, 1)
    nf, nl = _solve_on_graph(shim, 200, [(i, i + 1) for i in range(199)], 4)
    assert nf > 30 and nl > 4
    comp = [(i, i + 1) for i in range(39)] + [(40 + i, 41 + i) for i in range(39)]       # nodes 0..39 and 40..79
    assert _solve_on_graph(shim, 80, comp, 8)[0] > 5
    assert _solve_on_graph(shim, 24, [(i, j) for i in range(24) for j in range(i)], 4)[0] >= 1
