"""GPU checks of the modal solve: the block kernels and tlfea_newton_modal_solve against scipy on matrices
retrieved through the oracle-checked entry points (RetrieveHessianCSRToCPU, RetrieveMassCSRToCPU) -- never against the
modal code itself.

The dense reference is scipy.linalg.eigh of the reduced pencil.  The T10 mass matrix (5-point Keast rule, negative
centroid weight) is symmetric but not positive definite, so eigh(K, M) raises on it; the same pencil goes in as
eigh(M, A) with A = K + sigma M (SPD), eigenvalues theta = 1 / (omega^2 + sigma), the physical modes the largest.

Bars.  Residual: 2 tol (omega^2 + sigma) |M phi| (the solve stops at tol on its own fp64 sums; the factor 2 covers the
NumPy re-evaluation).  omega^2 against eigh: the residual bound puts the ceiling at 2 tol (omega^2 + sigma) = 2e-8; the
error is quadratic in the residual, so far less is expected.  Each comparison has its own bar, ten times the gap measured
for it on an MI355X (GAP_BAR below, relative to omega^2 + sigma; the measured values are beside the bars).
"""
import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_gpu, tl
from tests.test_gpu_ancf import SVK as ANCF_SVK, beam_problem, make_pair, plate_problem

pytestmark = pytest.mark.gpu
TOL = 1e-8
CAP = 500
SIGMA = (2 * np.pi) ** 2
# ten times the measured gap of each comparison, relative to omega^2 + sigma; every one below the ceiling 2 * TOL
GAP_BAR = {"beam_svk": 5.2e-13,      # measured 5.2e-14
           "beam_neo": 1.2e-12,      # 1.2e-13
           "cube": 5.3e-11,          # elastic modes 7-10 of the free cube: 5.3e-12 at either shift
           "beam3243": 3.0e-12,      # ANCF-3243 cantilever 3.0e-13
           "plate3443": 3.0e-9,      # ANCF-3443 plate 3.0e-10 (276 iterations: bending of a thin plate next to its membrane stiffness)
           "tension": 7.2e-13,       # 7.2e-14
           "floor": 4.2e-13}         # beam resting on a frictionless plane: 4.2e-14


def newton(d, h=1e-3):
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-6, 0.0, 1e-6, 1e14, 5, 10, h))
    return s


def free_mask(d, fixed):
    free = np.ones(3 * d.get_n_coef(), dtype=bool)
    if fixed is not None and len(fixed):
        free[(3 * np.asarray(fixed)[:, None] + np.arange(3)).reshape(-1)] = False
    return free


def retrieved(s, d):
    """H (at the solver's time step) and M (x) I3 as scipy CSR"""
    n = 3 * d.get_n_coef()
    s.AssembleHessian()
    ro, ci, val = s.RetrieveHessianCSRToCPU()
    H = sp.csr_matrix((val, ci, ro), shape=(n, n))
    off, col, mv = d.RetrieveMassCSRToCPU()
    M = sp.kron(sp.csr_matrix((mv, col, off), shape=(n // 3, n // 3)), sp.identity(3)).tocsr()
    return H, M


def dense_reference(s, d, free, h, k):
    """K = (H - M / h) / h and M on the free DOFs (dense), and the k lowest omega^2 with M-normalised vectors by eigh"""
    H, M = retrieved(s, d)
    K = ((H - M / h) / h).toarray()[np.ix_(free, free)]
    Md = M.toarray()[np.ix_(free, free)]
    K, Md = 0.5 * (K + K.T), 0.5 * (Md + Md.T)
    th, V = sl.eigh(Md, K + SIGMA * Md)
    th, V = th[::-1][:k], V[:, ::-1][:, :k]
    return K, Md, 1.0 / th - SIGMA, V / np.sqrt(th)[None, :]


def check_modes(res, K, Md, w2_ref, V_ref, free, bar, sigma=SIGMA, tol=TOL, k_complete=True):
    k = len(res.omega2)
    assert res.converged == k and res.iterations <= CAP
    Phi = res.modes.reshape(k, -1).T
    assert not Phi[~free].any()
    Phi = Phi[free]
    MP = Md @ Phi
    R = K @ Phi - MP * res.omega2[None, :]
    rel = np.linalg.norm(R, axis=0) / ((res.omega2 + sigma) * np.linalg.norm(MP, axis=0))
    gap = np.abs(res.omega2 - w2_ref) / (w2_ref + sigma)
    orth = np.abs(Phi.T @ MP - np.eye(k)).max()
    print(f"  iterations {res.iterations} precond {res.precond} block {res.block}\n  omega2 {res.omega2}\n"
          f"  independent residual {rel.max():.3e}  reported {res.residuals.max():.3e}  gap {gap.max():.3e}  orth {orth:.3e}")
    assert np.all(rel <= 2 * tol)
    assert orth <= 1e-10
    assert np.all(gap <= bar)
    # M-inner product with the scipy vectors: |cos| >= 1 - 1e-8 for a simple eigenvalue; a degenerate group (relative
    # distance below 1e-6: the two bending planes of a square cross-section) as a subspace -- what the projection on the
    # scipy group leaves of the computed vectors.  A group cut by the end of the list is not compared.
    groups, g = [], [0]
    for i in range(1, k):
        if abs(w2_ref[i] - w2_ref[g[-1]]) <= 1e-6 * (w2_ref[i] + sigma):
            g.append(i)
        else:
            groups.append(g)
            g = [i]
    groups.append(g)
    for g in groups:
        C = V_ref[:, g].T @ MP[:, g]
        left = np.abs(C.T @ C - np.eye(len(g))).max()
        print(f"  modes {g}: 1 - |cos|^2 or projection residual {left:.2e}")
        if len(g) == 1:
            assert abs(C[0, 0]) >= 1 - 1e-8
        elif g[-1] < k - 1 or k_complete:
            assert left <= 2e-8
    return Phi, MP


def beam(mat="svk", f_ext=None):
    X, conn = load_mesh("beam_3x2x1")
    fixed = fixed_x0(X)
    return X, conn, fixed, make_gpu(X, conn, MATERIALS[mat], fixed, f_ext)


# ---- 1, 2: the block kernels ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def beam_solver():
    X, conn, fixed, d = beam()
    s = newton(d)
    H, M = retrieved(s, d)
    yield dict(d=d, s=s, H=H, M=M, free=free_mask(d, fixed), n=3 * X.shape[0])
    del s
    d.Destroy()


@pytest.mark.parametrize("m", [1, 3, 8, 17, 32])
@pytest.mark.parametrize("mask", [False, True])
def test_block_products(beam_solver, m, mask):
    b = beam_solver
    X = np.random.default_rng(m).normal(size=(b["n"], m))
    for which, A in ((0, b["H"]), (1, b["M"])):
        Y = b["s"].ModalApplyBlock(X, which, mask)
        ref = A @ X
        if mask:
            ref[~b["free"]] = 0.0
        err = np.linalg.norm(Y - ref, axis=0) / np.linalg.norm(ref, axis=0)
        print(f"  which {which} m {m} mask {mask}: column-wise relative error {err.max():.2e}")
        assert np.all(err <= 1e-13)
        assert np.array_equal(Y, b["s"].ModalApplyBlock(X, which, mask))


@pytest.mark.parametrize("p,q", [(1, 1), (3, 24), (96, 96), (17, 5)])
def test_gram(beam_solver, p, q):
    b = beam_solver
    rng = np.random.default_rng(100 * p + q)
    X, Y = rng.normal(size=(b["n"], p)), rng.normal(size=(b["n"], q))
    G = b["s"].ModalGram(X, Y)
    bound = 1e-13 * np.outer(np.linalg.norm(X, axis=0), np.linalg.norm(Y, axis=0))
    print(f"  ({p}, {q}): max error / bound {np.max(np.abs(G - X.T @ Y) / bound):.2e}")
    assert np.all(np.abs(G - X.T @ Y) <= bound)
    assert np.array_equal(G, b["s"].ModalGram(X, Y))
    _, _, _, d2 = beam()
    s2 = newton(d2)
    assert np.array_equal(G, s2.ModalGram(X, Y))
    del s2
    d2.Destroy()


# ---- 3: clamped T10 beam --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mat", ["svk", "neo"])
def test_clamped_beam(mat):
    X, conn, fixed, d = beam(mat)
    s = newton(d)
    free = free_mask(d, fixed)
    K, Md, w2, V = dense_reference(s, d, free, 1e-3, 6)
    res = s.ModalAnalysis(6, tol=TOL, max_iter=CAP)
    assert res.precond == s.GetPreconditioner()
    check_modes(res, K, Md, w2, V, free, GAP_BAR["beam_" + mat])
    assert np.allclose(res.freq_hz, np.sqrt(res.omega2) / (2 * np.pi))
    del s
    d.Destroy()


# ---- 4: free T10 cube -----------------------------------------------------------------------------------------------
def test_free_cube():
    X, conn = load_mesh("cube")
    d = make_gpu(X, conn, MATERIALS["svk"])
    s = newton(d)
    free = free_mask(d, None)
    K, Md, w2, V = dense_reference(s, d, free, 1e-3, 10)
    out = []
    for sigma in (SIGMA, 4 * SIGMA):
        res = s.ModalAnalysis(10, shift=sigma, tol=TOL, max_iter=CAP)
        print(f"  shift {sigma:.4g}: iterations {res.iterations} omega2 {res.omega2}")
        assert res.converged == 10
        assert np.all(np.abs(res.omega2[:6]) <= 1e-8 * res.omega2[6])
        gap = np.abs(res.omega2[6:] - w2[6:]) / (w2[6:] + sigma)
        print(f"  gap of the elastic modes {gap.max():.3e}")
        assert np.all(gap <= GAP_BAR["cube"])
        Phi = res.modes.reshape(10, -1).T
        MP = Md @ Phi
        assert np.abs(Phi.T @ MP - np.eye(10)).max() <= 1e-10
        R = K @ Phi - MP * res.omega2[None, :]
        assert np.all(np.linalg.norm(R, axis=0) <= 2 * TOL * (res.omega2 + sigma) * np.linalg.norm(MP, axis=0))
        # degenerate groups (the rigid-body modes; elastic modes closer than 1e-6 relative) as subspaces: what is left of
        # the computed vectors after projection on the scipy group, in the M-inner product
        groups, g = [list(range(6))], [6]
        for i in range(7, 10):
            if abs(w2[i] - w2[g[-1]]) <= 1e-6 * w2[i]:
                g.append(i)
            else:
                groups.append(g)
                g = [i]
        groups.append(g)
        for g in groups:
            C = V[:, g].T @ MP[:, g]
            left = np.abs(C.T @ C - np.eye(len(g))).max()
            print(f"  group {g}: projection residual {left:.2e}")
            assert left <= (1e-6 if g[0] == 0 else 2e-8)
        out.append(res.omega2)
    # two results that each lie within the bar of eigh lie within twice the bar of each other
    assert np.all(np.abs(out[0][6:] - out[1][6:]) <= 2 * GAP_BAR["cube"] * (w2[6:] + 4 * SIGMA))
    del s
    d.Destroy()


# ---- 5: ANCF (Chebyshev / 12 x 12 node-block path of T) --------------------------------------------------------------
@pytest.mark.parametrize("pname", ["beam3243", "plate3443"])
def test_ancf(pname):
    prob = beam_problem(n_elem=4) if pname == "beam3243" else plate_problem()
    _, d = make_pair(prob, ANCF_SVK)
    fixed = prob[6]
    s = newton(d)
    free = free_mask(d, fixed)
    K, Md, w2, V = dense_reference(s, d, free, 1e-3, 4)
    res = s.ModalAnalysis(4, tol=TOL, max_iter=CAP)
    assert res.precond == 1
    print("  polynomial", s.GetPolynomialInfo())
    check_modes(res, K, Md, w2, V, free, GAP_BAR[pname])
    del s
    d.Destroy()


# ---- 6: prestress ---------------------------------------------------------------------------------------------------
def test_prestress_raises_the_first_frequency():
    X, conn, fixed, d = beam()
    s = newton(d)
    w2_0 = s.ModalAnalysis(1, tol=TOL, max_iter=CAP).omega2[0]
    del s
    d.Destroy()
    X, conn, fixed, d = beam()
    bf = d.GetBoundaryFaces()
    d.AddFaceTraction(np.nonzero(bf.normal[:, 0] > 0.99)[0], np.array([5e6, 0.0, 0.0]))   # axial tension, dead
    h = 1.0                                                                               # quasi-static steps to rest
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 0.0, 1e-6, 1e14, 5, 30, h))
    for _ in range(6):
        s.Solve()
    assert np.abs(s.RetrieveVelocityToCPU()).max() < 1e-6
    free = free_mask(d, fixed)
    K, Md, w2, V = dense_reference(s, d, free, h, 3)
    res = s.ModalAnalysis(3, tol=TOL, max_iter=CAP)
    print(f"  omega_1^2 unloaded {w2_0:.6f} in tension {res.omega2[0]:.6f}")
    check_modes(res, K, Md, w2, V, free, GAP_BAR["tension"])
    assert res.omega2[0] > 1.05 * w2_0
    del s
    d.Destroy()


# ---- 7, 8: no side effects, reproducibility ------------------------------------------------------------------------------
def test_no_side_effects_and_reproducible():
    f_ext = np.zeros(3 * 105)
    f_ext[3 * 19] = 2.0e5
    runs = []
    for modal in (False, True, True):
        X, conn, fixed, d = beam(f_ext=f_ext)
        s = newton(d)
        s.Solve()
        res = None
        if modal:
            res = s.ModalAnalysis(6, tol=TOL, max_iter=CAP)
            _, _, after = s.RetrieveHessianCSRToCPU()
            s.AssembleHessian()
            assert np.array_equal(after, s.RetrieveHessianCSRToCPU()[2])
        s.Solve()
        runs.append((np.stack(d.RetrievePositionToCPU()), s.RetrieveVelocityToCPU(), s.RetrieveLambdaToCPU(), res))
        del s
        d.Destroy()
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(runs[1][3].omega2, runs[2][3].omega2) and np.array_equal(runs[1][3].modes, runs[2][3].modes)
    assert runs[1][3].iterations == runs[2][3].iterations


# ---- 9: refusals ------------------------------------------------------------------------------------------------------
def _refusal_cases():
    def damped(d, s):
        d.SetDamping(1e4, 0.0)

    def table(d, s):
        mats = [tl.ElementMaterial(E=7e8, nu=0.33, rho0=2700.0), tl.ElementMaterial(E=7e8, nu=0.33, rho0=2700.0, eta=1e4)]
        d.SetElementMaterials(np.arange(d.get_n_elem()) % 2, mats)
        d.CalcMassMatrix()

    def iface(d, s):
        s.SetInterface(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.ones(d.get_n_coef()), lambda p, n: None)

    def direct(d, s):
        s.SetLinSolveOpts(tl.LinSolveOpts(method=1))

    def friction(d, s):
        d.SetRigidObstacles([tl.RigidPlane((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 1e9, friction=0.3)])

    return [("damping", damped, dict(n_modes=6), "damping"), ("table", table, dict(n_modes=6), "damping"),
            ("interface", iface, dict(n_modes=6), "partitioned"), ("direct", direct, dict(n_modes=6), "method = 1"),
            ("friction", friction, dict(n_modes=6), "friction"),
            ("shift0", None, dict(n_modes=6, shift=0.0), "shift"), ("shiftnan", None, dict(n_modes=6, shift=np.nan), "shift"),
            ("shiftneg", None, dict(n_modes=6, shift=-1.0), "shift"), ("shiftinf", None, dict(n_modes=6, shift=np.inf), "shift"),
            ("nmodes", None, dict(n_modes=0), "n_modes"), ("block", None, dict(n_modes=20, block_extra=13), "exceeds 32"),
            ("dofs", None, dict(n_modes=32, block_extra=0), "free DOFs")]


@pytest.mark.parametrize("case", _refusal_cases(), ids=lambda c: c[0])
def test_refusals_leave_the_solver_usable(case):
    name, prepare, kw, word = case
    f_ext = np.zeros(3 * 105)
    f_ext[3 * 19] = 2.0e5
    out = []
    for refused in (False, True):
        if name == "dofs":     # 3 x 32 = 96 columns against the 81 DOFs of the free cube
            X, conn = load_mesh("cube")
            d = make_gpu(X, conn, MATERIALS["svk"], None, np.r_[1e4, np.zeros(80)])
        else:
            X, conn, fixed, d = beam(f_ext=f_ext)
        s = newton(d)
        if prepare:
            prepare(d, s)
        if refused:
            with pytest.raises(tl.TlfeaError, match=word):
                s.ModalAnalysis(**kw)
        s.Solve()
        out.append((np.stack(d.RetrievePositionToCPU()), s.RetrieveVelocityToCPU()))
        del s
        d.Destroy()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_refusal_without_a_mass_matrix():
    X, conn = load_mesh("beam_3x2x1")
    q = tl.quadrature
    d = tl.GPU_FEAT10_Data(conn.shape[0], X.shape[0])
    d.Initialize()
    d.Setup(q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights, X[:, 0], X[:, 1], X[:, 2], conn)
    d.SetDensity(2700.0)
    d.SetSVK(7e8, 0.33)
    d.CalcDnDuPre()
    s = newton(d)
    with pytest.raises(tl.TlfeaError, match="mass matrix"):
        s.ModalAnalysis(4)
    d.CalcMassMatrix()
    assert s.ModalAnalysis(4, shift=1e4).converged == 4     # a free beam: six rigid-body modes come first
    del s
    d.Destroy()


def test_refusal_with_an_overlapping_partition():
    """set_halo: the one-rank partition (every node owned, no peers) switches the solver to the partitioned path"""
    part_mod = __import__("importlib").import_module("total-lagrangian-fea_amd.partition")
    X, conn, fixed, d = beam()
    s = newton(d)
    part = part_mod.halo_partition(X, conn, np.zeros(X.shape[0], dtype=np.int32), np.arange(X.shape[0]), 0, 1, 3)
    assert np.array_equal(part.l2g, np.arange(X.shape[0]))
    s.SetHalo(part, allreduce=lambda p, n: None, exchange=lambda *a: None)
    with pytest.raises(tl.TlfeaError, match="partitioned"):
        s.ModalAnalysis(6)
    del s
    d.Destroy()


# ---- contact stiffness of a frictionless obstacle ------------------------------------------------------------------------
def test_beam_resting_on_a_frictionless_plane():
    """The clamped beam with a rigid plane 1 mm above its bottom face (z = 0): the penalty stiffness of the surface nodes in
    contact is part of K, raises omega_1^2 and is the same at two shifts; against eigh on the matrices retrieved at that
    state, as every other case."""
    X, conn, fixed, d = beam()
    s = newton(d)
    w2_0 = s.ModalAnalysis(1, tol=TOL, max_iter=CAP).omega2[0]
    d.SetRigidObstacles([tl.RigidPlane((0.0, 0.0, 1e-3), (0.0, 0.0, 1.0), 1e9)])
    free = free_mask(d, fixed)
    K, Md, w2, V = dense_reference(s, d, free, 1e-3, 4)
    res = s.ModalAnalysis(4, tol=TOL, max_iter=CAP)
    print(f"  omega_1^2 free {w2_0:.6f} on the plane {res.omega2[0]:.6f}")
    check_modes(res, K, Md, w2, V, free, GAP_BAR["floor"])
    assert res.omega2[0] > 1.05 * w2_0
    res2 = s.ModalAnalysis(4, shift=4 * SIGMA, tol=TOL, max_iter=CAP)
    assert np.all(np.abs(res2.omega2 - res.omega2) <= 2 * GAP_BAR["floor"] * (w2 + 4 * SIGMA))   # each within the bar of eigh
    del s
    d.Destroy()


# ---- the host driver -------------------------------------------------------------------------------------------------
def test_beam_modes_driver(tmp_path):
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "total-lagrangian-fea_amd", "host", "test_beam_modes")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    vtu = tmp_path / "beam_modes.vtu"
    p = subprocess.run(["timeout", "-k", "10", "120", exe, "--mesh_dir=" + os.path.join(root, "tests", "golden", "meshes"),
                        "--vtu=" + str(vtu)], capture_output=True, text=True, timeout=140)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    printed = re.findall(r"^Mode \d+: f=(\S+) Hz", p.stdout, re.M)
    assert len(printed) == 6
    X, conn = load_mesh("res4")
    fixed = fixed_x0(X)
    d = make_gpu(X, conn, MATERIALS["svk"], fixed)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(1e-4, 1e-4, 1e-4, 1e14, 5, 10, 1e-3))
    res = s.ModalAnalysis(6)
    print(p.stdout)
    assert printed == ["%.9e" % f for f in res.freq_hz]          # equal to the printed digits
    txt = vtu.read_text()
    n = int(re.search(r'NumberOfPoints="(\d+)"', txt).group(1))
    assert n == X.shape[0]
    for k in range(6):
        body = re.search(r'<DataArray type="Float64" Name="mode_%d"[^>]*>\n(.*?)</DataArray>' % k, txt, re.S).group(1)
        rows = np.array([[float(v) for v in ln.split()] for ln in body.splitlines() if ln.strip()])
        assert rows.shape == (n, 3) and np.allclose(rows, res.modes[k], rtol=1e-12, atol=1e-300)
    fd = re.search(r'<FieldData>.*?Name="frequency_hz" NumberOfTuples="6"[^>]*>\n(.*?)</DataArray>', txt, re.S).group(1)
    assert np.allclose([float(v) for v in fd.split()], res.freq_hz, rtol=1e-13)
    del s
    d.Destroy()
