"""tests/fine_matfree_np.py on H from the oracle, without a GPU.  The fine pass is restated as the device forms it -- the
element map of tests/matfree_np.py evaluated in float32 on float32 records, with the device's normalisation, then the
polynomial step's epilogue -- and the cycle wraps tests/precond_np.py / tests/restricted_op_np.py around it with R from
the exact operator, rounded to float32.  On every mesh tests/test_gpu_fine_matfree.py uses: the element map in float64 is
H itself, the fp32 floor of the operator (float32 against float64 work vectors) is at most 1e-4, and the restated
cycle's own symmetry defect stays within 8 x that floor -- the bound the device is then held to.  The same floor at both
ends of the range of units (E = 1e12 Pa with h = 1e-5, E = 1e3 Pa with h = 1e-1): nothing overflows or flushes to zero."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import fine_matfree_np as fm
from tests import galerkin_np as gn
from tests import precond_np as pn
from tests.helpers import MATERIALS, fixed_x0, make_oracle, tl

EDGES = [(0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3)]
NU, RHO_PEN = 0.33, 1e14


def lam_max(level, its=60):
    """largest eigenvalue of (S D S)^-1 Hs by power iteration (the meshes here are too large for dense eigenvalues)"""
    v = np.random.default_rng(1).normal(size=level.n)
    lam = 0.0
    for _ in range(its):
        w = level.dinv(level.Hs @ v)
        lam = float(np.linalg.norm(w) / np.linalg.norm(v))
        v = w / np.linalg.norm(w)
    return lam


def build(name, E, h):
    """H at a perturbed state with x = 0 pinned and Kelvin-Voigt damping on, the element records and the vertex hierarchy"""
    X, conn = gn.mesh(name)
    fixed = fixed_x0(X)
    m = dict(MATERIALS["svk_damped"], E=E, nu=NU, eta=1e-4 * E * h, lamd=1e-4 * E * h)
    o = make_oracle(X, conn, m, fixed)
    x = X + np.random.default_rng(7).normal(0.0, 1e-4, X.shape)
    x[fixed] = X[fixed]
    o.x, o.y, o.z = (np.ascontiguousarray(x[:, i]) for i in range(3))
    ro, ci, val = o.assemble_hessian(h, RHO_PEN)
    N = X.shape[0]
    H = sp.csr_matrix((val, ci, ro), shape=(3 * N, 3 * N))
    q = tl.quadrature
    ep = fm.element_problem(X, conn, x, (q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights), E, NU, m["rho0"], h, m["eta"],
                            m["lamd"], fixed, RHO_PEN)
    verts = np.unique(conn[:, :4])
    cid = -np.ones(N, dtype=np.int64)
    cid[verts] = np.arange(len(verts))
    par0, par1 = cid.copy(), cid.copy()
    for k, (a, b) in enumerate(EDGES):
        par0[conn[:, 4 + k]], par1[conn[:, 4 + k]] = cid[conn[:, a]], cid[conn[:, b]]
    P = pn.prolongation_p(par0, par1, len(verts))
    data = dict(ep, par0=par0, par1=par1, **pn.pack_csr("H", H), **pn.pack_csr("Hc", (P.T @ H @ P).tocsr()))
    return dict(name=name, H=H, data=data, n=3 * N)


def cycle_states(p):
    f, c = fm.fine_level(p["H"]), pn.Level(pn.unpack_csr("Hc", p["data"]), fm.COARSE_STORE)
    lf, lc = 1.15 * lam_max(f), 1.15 * lam_max(c)
    out = {}
    for ks, kappa in ((2, 8.0), (4, 24.0)):
        st = pn.cycle_state(pn.chebyshev_pairs(lf, kappa, ks), pn.chebyshev_pairs(lc, 216.0, 12))
        st.update(precond=2, levels=2, smoother=1)
        out[ks] = st
    return out


def floor_and_symmetry(p, st):
    op64, op32 = fm.element_operator_from(p["data"], st, np.float64), fm.element_operator_from(p["data"], st, np.float32)
    floor = 0.0
    for r in np.random.default_rng(11).normal(size=(3, p["n"])):
        z64 = op64(r)
        assert np.all(np.isfinite(op32(r)))
        floor = max(floor, float(np.linalg.norm(op32(r) - z64) / np.linalg.norm(z64)))
    return floor, fm.symmetry_defect(op64, p["n"])


@pytest.fixture(scope="module", params=gn.MESHES)
def problem(request):
    return build(request.param, MATERIALS["svk_damped"]["E"], 1e-3)


def test_element_map_in_float64_is_the_scaled_matrix(problem):
    p = problem
    L = fm.ElementLevel(p["H"], p["data"])
    for d in np.random.default_rng(2).normal(size=(2, p["n"])):
        ref = L.Hs @ d
        assert np.abs(L.hs(d) - ref).max() <= 1e-11 * np.abs(ref).max()


@pytest.mark.parametrize("ks", [2, 4])
def test_floor_and_symmetry_of_the_restated_cycle(problem, ks):
    floor, sym = floor_and_symmetry(problem, cycle_states(problem)[ks])
    print(problem["name"], "ks", ks, "floor %.2e symmetry defect %.2e" % (floor, sym))
    assert 0.0 < floor <= 1e-4, floor
    assert sym <= 8.0 * floor, (sym, floor)


@pytest.mark.parametrize("E,h", [(1e12, 1e-5), (1e3, 1e-1)], ids=["stiff", "soft"])
def test_range_of_units(E, h):
    """the float32 pass at both ends: every intermediate of the normalised map stays a normal float32"""
    p = build("box", E, h)
    L32, L64 = fm.ElementLevel(p["H"], p["data"], np.float32), fm.ElementLevel(p["H"], p["data"])
    tiny = np.finfo(np.float32).tiny
    for v in (L32.scn, L32.g, L32.detJ, L32.F, np.array(L32.k[:4]), np.array([L32.tau, L32.pen])):
        a = np.abs(np.asarray(v, dtype=np.float64))
        assert np.all(np.isfinite(a)) and np.all((a == 0.0) | (a >= tiny)), (E, h)
    d = np.random.default_rng(4).normal(size=p["n"]).astype(np.float32)
    y32, y64 = L32.hs(d), L64.hs(d.astype(np.float64))
    assert np.all(np.isfinite(y32)) and np.abs(y32 - y64).max() <= 1e-5 * np.abs(y64).max()
    floor, sym = floor_and_symmetry(p, cycle_states(p)[2])
    print("E %g h %g floor %.2e symmetry defect %.2e" % (E, h, floor, sym))
    assert 0.0 < floor <= 1e-4 and sym <= 8.0 * floor, (floor, sym)


def test_r_from_h_is_the_restricted_exact_operator(problem):
    """R of the exact fine level is S_c P^T H S_f: the quotient by S_f cancels against Hs = S_f H S_f"""
    from tests import restricted_op_np as rn
    p = problem
    Hc = pn.unpack_csr("Hc", p["data"])
    f, c = fm.fine_level(p["H"]), pn.Level(Hc, fm.COARSE_STORE)
    P = pn.prolongation_p(p["data"]["par0"], p["data"]["par1"], Hc.shape[0] // 3)
    R = rn.restricted_operator(f, c, P, 64)
    ref = (sp.diags(c.sc) @ P.T @ p["H"] @ sp.diags(f.sc)).tocsr()
    assert abs(R - ref).max() <= 1e-12 * abs(ref).max()
