"""Stress and energy recovery of ANCF beam and shell meshes on the GPU (DESIGN 3f'), through the Python mirror, against
tests/ancf_stress_np.py (pinned without a GPU by tests/test_ancf_stress_np.py).  The shapes sit where the lane mapping
can go wrong: beams E = 1, 5, 6 (part of a wavefront's five elements, exactly five, the first element of a second
wavefront) and the welded 20 x 20 net; shells E = 1, a 2 x 2 plate (a node of four elements), a 3 x 1 strip."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ancf_stress_np as anp
from tests import stress_np as snp
from tests.helpers import MATERIALS, load_mesh, make_gpu, tl
from tests.test_linear_constraints import NET_W, TIRE

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
Q = tl.quadrature
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
SHAPES = {"beam1": lambda: anp.beam_line(1), "beam5": lambda: anp.beam_line(5), "beam6": lambda: anp.beam_line(6),
          "net": lambda: anp.net(NET_W), "shell1": lambda: anp.shell_plate(1, 1), "plate2x2": lambda: anp.shell_plate(2, 2),
          "strip3x1": lambda: anp.shell_plate(3, 1)}
MATS = ("svk", "mr", "svk_damped", "mr_damped")
FIELDS = ("point_sigma", "elem_sigma", "elem_von_mises", "elem_psi", "elem_J", "elem_volume", "nodal_sigma", "nodal_von_mises")
TOTALS = ("strain_energy", "viscous_power", "reference_volume", "current_volume")


def make_ancf_gpu(prob, m, mass=True):
    kind, x, y, z, conn, (L, W, H) = prob
    d = (tl.GPU_ANCF3243_Data if kind == 3243 else tl.GPU_ANCF3443_Data)(len(x) // 4, conn.shape[0])
    d.Initialize()
    if kind == 3243:
        d.Setup(L, W, H, Q.gauss_xi_m_6, Q.gauss_xi_3, Q.gauss_eta_2, Q.gauss_zeta_2, Q.weight_xi_m_6, Q.weight_xi_3,
                Q.weight_eta_2, Q.weight_zeta_2, x, y, z, conn)
    else:
        d.Setup(L, W, H, Q.gauss_xi_m_7, Q.gauss_eta_m_7, Q.gauss_zeta_m_3, Q.gauss_xi_4, Q.gauss_eta_4, Q.gauss_zeta_3,
                Q.weight_xi_m_7, Q.weight_eta_m_7, Q.weight_zeta_m_3, Q.weight_xi_4, Q.weight_eta_4, Q.weight_zeta_3,
                x, y, z, conn)
    d.SetDensity(m["rho0"])
    d.SetDamping(m["eta"], m["lamd"])
    if m["kind"] == "svk":
        d.SetSVK(m["E"], m["nu"])
    else:
        d.SetMooneyRivlin(m["mu10"], m["mu01"], m["kappa"])
    d.CalcDsDuPre()
    if mass:
        d.CalcMassMatrix()
    return d


@functools.lru_cache(maxsize=None)
def reference(shape, mat):
    """(oracle, x, v, restated fields) of a shape at its perturbed state: computed once, shared, never modified"""
    m = MATERIALS[mat]
    o = anp.make_oracle(SHAPES[shape](), m)
    x, v = anp.perturbed(o)
    return o, x, v, anp.recover(o, m, x, v)


def move(d, x):
    d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])


def fields(d, points=True):
    e, n, t = d.RetrieveANCFElementStressToCPU(), d.RetrieveANCFNodalStressToCPU(), d.GetANCFEnergies()
    out = dict(elem_sigma=e.sigma, elem_von_mises=e.von_mises, elem_psi=e.psi, elem_J=e.J, elem_volume=e.volume,
               nodal_sigma=n.sigma, nodal_von_mises=n.von_mises, strain_energy=t.strain, kinetic=t.kinetic,
               viscous_power=t.viscous_power, reference_volume=t.reference_volume, current_volume=t.current_volume)
    if points:
        out["point_sigma"] = d.RetrieveANCFPointStressToCPU()
    return out


# ---- 1. parity with the restatement (the tolerances of tests/test_gpu_stress.py::test_parity_with_restatement) ----------
@pytest.mark.parametrize("mat", MATS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_parity_with_restatement(shape, mat):
    m = MATERIALS[mat]
    o, x, v, ref = reference(shape, mat)
    d = make_ancf_gpu(SHAPES[shape](), m)
    move(d, x)
    d.CalcElementStress(v, want_points=True)
    got = fields(d)
    assert got["nodal_sigma"].shape == (o.N // 4, 6) and got["point_sigma"].shape == (o.E, o.Q, 6)
    for name in FIELDS:
        scale = np.abs(ref[name]).max()
        err = np.abs(got[name] - ref[name]).max()
        print(f"{shape} {mat} {name}: {err / scale:.2e}")
        assert err <= 1e-10 * scale, name
    floor = {"strain_energy": 256 * EPS * anp.moduli(m) * ref["reference_volume"]}
    for name in TOTALS:
        err = abs(got[name] - ref[name])
        print(f"{shape} {mat} {name}: {got[name]:.15e} vs {ref[name]:.15e}")
        assert err <= 1e-12 * abs(ref[name]) + floor.get(name, 0.0), name
    assert abs(got["kinetic"] - ref["kinetic"]) <= 1e-12 * ref["kinetic"]
    if m["eta"] != 0:
        assert got["viscous_power"] > 0
    else:
        assert got["viscous_power"] == 0.0
    d.CalcElementStress()                                        # without a velocity: elastic stress, no kinetic energy
    t = d.GetANCFEnergies()
    assert t.kinetic == 0.0 and t.viscous_power == 0.0
    assert abs(t.strain - ref["strain_energy"]) <= 1e-12 * abs(ref["strain_energy"]) + floor["strain_energy"]
    d.Destroy()


# ---- 2. known answers through the GPU path -------------------------------------------------------------------------------
@pytest.mark.parametrize("mat", ["svk", "mr"])
@pytest.mark.parametrize("shape", ["beam6", "plate2x2"])
def test_affine_map_and_rigid_rotation(shape, mat):
    m, prob, A = MATERIALS[mat], SHAPES[shape](), anp.A_STRETCH
    X = np.stack(prob[1:4], axis=1)
    V = prob[4].shape[0] * np.prod(prob[5])
    d = make_ancf_gpu(prob, m, mass=False)
    move(d, X @ A.T)
    d.CalcElementStress(want_points=True)
    got = fields(d)
    s_ref = anp.cauchy_closed_form(A, m)
    tol = 1e-12 * np.abs(s_ref).max() + 256 * EPS * anp.moduli(m)     # tests/test_gpu_stress.py::test_homogeneous_deformation
    for name in ("point_sigma", "elem_sigma", "nodal_sigma"):
        assert np.abs(got[name] - s_ref).max() <= tol, name
    assert np.abs(got["nodal_von_mises"] - snp.von_mises(s_ref)).max() <= 2 * tol
    assert abs(got["reference_volume"] - V) <= 1e-12 * V
    assert abs(got["current_volume"] - np.linalg.det(A) * V) <= 1e-12 * V
    W = float(snp.psi(A, m)) * V
    assert abs(got["strain_energy"] - W) <= 1e-12 * W + 256 * EPS * anp.moduli(m) * V
    move(d, X @ anp.Q_ROT.T)
    d.CalcElementStress(want_points=True)
    rigid = fields(d)
    K = anp.moduli(m)                                                 # tests/test_gpu_stress.py::test_objectivity
    assert np.abs(rigid["point_sigma"]).max() <= 1e-9 * K
    assert np.abs(rigid["nodal_von_mises"]).max() <= 1e-9 * K
    assert abs(rigid["strain_energy"]) <= 1e-9 * K * V
    d.Destroy()


# ---- 3. determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["beam6", "net", "plate2x2"])
def test_bitwise_reproducible_and_independent_of_want_points(shape):
    m = MATERIALS["mr_damped"]
    _, x, v, _ = reference(shape, "mr_damped")
    runs = []
    for _ in range(2):
        d = make_ancf_gpu(SHAPES[shape](), m)
        move(d, x)
        for points in (True, False, True):
            d.CalcElementStress(v, want_points=points)
            f = fields(d, points)
            runs.append({k: np.asarray(f[k]) for k in f})
        d.Destroy()
    for r in runs[1:]:
        for k in r:
            assert np.array_equal(runs[0][k], r[k]), k


# ---- 4. the strain energy's derivative is the internal force ------------------------------------------------------------
@pytest.mark.parametrize("mat", ["svk", "mr"])
@pytest.mark.parametrize("shape", ["beam6", "plate2x2"])
def test_energy_derivative_is_the_internal_force(shape, mat):
    """Independent of the restated stress: a central difference of the GPU strain energy at +-eps along a random direction
    against RetrieveInternalForceToCPU() . dx.  eps = ancf_stress_np.FD_EPS = 1e-4 and the bound come from the same check on
    the NumPy reference for the same mesh, material and direction: 10 x its error, which is the truncation c eps^2 of the
    central difference (tests/test_ancf_stress_np.py: halving eps divides it by 4.00).  Found on the reference, relative
    to f . dx: beam6 svk 1.1e-6, beam6 mr 2.2e-6, plate2x2 svk 3.5e-6, plate2x2 mr 3.0e-7."""
    m = MATERIALS[mat]
    o, x, _, _ = reference(shape, mat)

    def force_np(xx):
        anp.set_state(o, xx)
        return o.internal_force(None)

    fd_np, fdx_np, _ = anp.energy_fd(lambda xx: anp.recover(o, m, xx)["strain_energy"], force_np, x, anp.FD_EPS)
    bound = 10 * abs(fd_np - fdx_np)
    d = make_ancf_gpu(SHAPES[shape](), m, mass=False)

    def energy(xx):
        move(d, xx)
        d.CalcElementStress()
        return d.GetANCFEnergies().strain

    def force(xx):
        move(d, xx)
        d.CalcP()
        d.CalcInternalForce()
        return d.RetrieveInternalForceToCPU()

    fd, fdx, _ = anp.energy_fd(energy, force, x, anp.FD_EPS)
    print(f"{shape} {mat}: reference |fd - f.dx| = {abs(fd_np - fdx_np):.3e} ({abs(fd_np - fdx_np) / abs(fdx_np):.2e} of f.dx), "
          f"GPU {abs(fd - fdx):.3e}")
    assert abs(fd - fdx) <= bound
    d.Destroy()


# ---- 5. does not disturb a step ----------------------------------------------------------------------------------------
def test_does_not_disturb_a_newton_step():
    """The 3243 beam driver configuration of tests/test_gpu_ancf.py (cantilever, tip force, Kelvin-Voigt damping, the
    drivers' solver parameters): the same bits with CalcElementStress before and after every step as without."""
    from tests.test_gpu_ancf import SVK_D, beam_problem, make_pair
    out = []
    for with_stress in (False, True):
        _, d = make_pair(beam_problem(), SVK_D)
        s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
        s.Setup()
        s.SetParameters(tl.SyncedNewtonParams(1e-4, 0.0, 1e-6, 1e14, 5, 10, 1e-3))
        s.SetLinSolveOpts(tl.LinSolveOpts(1e-13, 50000, 10))
        s.AnalyzeHessianSparsity()
        for _ in range(2):
            if with_stress:
                d.CalcElementStress(s, want_points=True)
            s.Solve()
            if with_stress:
                d.CalcElementStress(s)
                assert d.GetANCFEnergies().kinetic > 0
        out.append((s.RetrieveVelocityToCPU(), np.stack(d.RetrievePositionToCPU())))
        del s
        d.Destroy()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.abs(out[0][0]).max() > 0


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    kind, x, y, z, conn, (L, W, H) = prob = anp.beam_line(2)
    d = tl.GPU_ANCF3243_Data(len(x) // 4, conn.shape[0])
    d.Initialize()
    d.Setup(L, W, H, Q.gauss_xi_m_6, Q.gauss_xi_3, Q.gauss_eta_2, Q.gauss_zeta_2, Q.weight_xi_m_6, Q.weight_xi_3,
            Q.weight_eta_2, Q.weight_zeta_2, x, y, z, conn)
    d.SetDensity(2700.0)
    d.SetSVK(7e8, 0.33)
    with pytest.raises(tl.TlfeaError, match="CalcDsDuPre"):
        d.CalcElementStress()
    d.CalcDsDuPre()
    for call in (d.RetrieveANCFElementStressToCPU, d.RetrieveANCFNodalStressToCPU, d.RetrieveANCFPointStressToCPU,
                 d.GetANCFEnergies):
        with pytest.raises(tl.TlfeaError, match="has not been called"):
            call()
    assert not d.GetANCFNodalStressDevicePtr()
    with pytest.raises(tl.TlfeaError, match="CalcMassMatrix"):
        d.CalcElementStress(np.zeros(3 * len(x)))
    d.CalcElementStress()                                        # works without a mass matrix or a solver
    assert d.GetANCFEnergies().reference_volume == pytest.approx(2 * L * W * H, rel=1e-12)
    assert d.GetANCFNodalStressDevicePtr()
    with pytest.raises(tl.TlfeaError, match="point stresses"):
        d.RetrieveANCFPointStressToCPU()
    with pytest.raises(ValueError, match="entries"):
        d.CalcElementStress(np.zeros(5))
    for call in (d.CalcStress, d.RetrieveNodalStressToCPU, d.RetrieveElementStressToCPU, d.GetEnergies):
        with pytest.raises(tl.TlfeaError, match="ANCF"):         # the T10 entry points keep refusing an ANCF object
            call()
    d.Destroy()
    # a T10 handle at the ancf_ entry points
    X, tets = load_mesh("cube")
    t = make_gpu(X, tets, MATERIALS["svk"])
    lib = tl.load_library()
    out = np.zeros(6 * X.shape[0])
    for rc in (lib.tlfea_ancf_calc_stress(t._h, None, 0), lib.tlfea_ancf_calc_stress_host(t._h, tl.binding.dp(np.zeros(3 * X.shape[0])), 0),
               lib.tlfea_ancf_retrieve_nodal_stress(t._h, tl.binding.dp(out), None), lib.tlfea_ancf_get_energies(t._h, tl.binding.dp(out)),
               lib.tlfea_ancf_time_stress_kernels(t._h, None, 0, 1, tl.binding.dp(out))):
        assert rc != 0 and re.search("T10", lib.tlfea_last_error().decode())
    assert not lib.tlfea_ancf_nodal_stress_device_ptr(t._h)
    t.CalcStress()                                               # and its own recovery is untouched
    assert t.GetEnergies().reference_volume > 0
    t.Destroy()


# ---- 7. driver ---------------------------------------------------------------------------------------------------------
def run_driver(tmp_path, name, extra):
    exe = os.path.join(HOST, "test_ancf3443_mesh_newton")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    vtu = tmp_path / name
    # --load_fz=100 as tests/test_gpu_driver.py: the contact stiffness at which the driver's Newton iterations converge
    p = subprocess.run(["timeout", "-k", "10", "300", exe, "--mesh=" + TIRE, "--steps=2", "--dt=1e-3", "--load_fz=100",
                        "--vtu=" + str(vtu)] + extra, capture_output=True, text=True, timeout=320)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return vtu


def test_tire_driver_with_and_without_stress(tmp_path):
    n_nodes = tl.mesh_utils.ReadANCF3443MeshFromFile(TIRE).n_nodes
    vtu = run_driver(tmp_path, "with", ["--stress"])
    txt = (vtu / "ancf3443_mesh_000000.vtu").read_text()
    pieces = re.findall(r'<Piece NumberOfPoints="(\d+)"[^>]*>(.*?)</Piece>', txt, re.S)
    on_nodes = [body for n, body in pieces if int(n) == n_nodes]
    assert len(on_nodes) == 1
    for body in [b for _, b in pieces]:                          # every piece carries both arrays, one tuple per point
        n = int(re.search(r'<DataArray type="Float64" NumberOfComponents="3" format="ascii">\n(.*?)</DataArray>', body, re.S)
                .group(1).count("\n"))
        for name, comps in (("stress", 6), ("von_mises", 1)):
            rows = [ln for ln in re.search(r'<DataArray type="Float64" Name="%s"[^>]*>\n(.*?)</DataArray>' % name, body, re.S)
                    .group(1).splitlines() if ln.strip()]
            assert len(rows) == n and all(len(r.split()) == comps for r in rows), name
            assert np.all(np.isfinite(np.array([r.split() for r in rows], dtype=float)))
    rows = [ln for ln in re.search(r'Name="von_mises"[^>]*>\n(.*?)</DataArray>', on_nodes[0], re.S).group(1).splitlines() if ln.strip()]
    assert len(rows) == n_nodes
    csv = (vtu / "stress.csv").read_text().splitlines()
    assert csv[0] == "step,strain_energy,kinetic_energy,viscous_power,von_mises_max" and len(csv) == 3
    val = np.array([ln.split(",") for ln in csv[1:]], dtype=float)
    assert np.all(np.isfinite(val)) and np.all(val[:, 1] > 0) and np.all(val[:, 2] > 0) and np.all(val[:, 4] > 0)
    plain = run_driver(tmp_path, "without", [])
    assert sorted(os.listdir(plain)) == ["ancf3443_mesh_000000.vtu"]     # no new CSV
    ptxt = (plain / "ancf3443_mesh_000000.vtu").read_text()
    assert "stress" not in ptxt and "von_mises" not in ptxt and "PointData" not in ptxt and ptxt.count("<Piece") == 1
    # the frame's geometry is the one of the run with the flag
    assert re.search(r"<Points>.*?</Points>", ptxt, re.S).group(0) == re.search(r"<Points>.*?</Points>", txt, re.S).group(0)
