"""Stress and energy recovery on the GPU, through the Python mirror: parity with tests/stress_np.py fed with
the GPU's own F, the force-stress identity against the oracle-pinned force path, homogeneous deformation and rigid
rotation, per-element materials, energies after Newton steps, no disturbance of a step, determinism, the refusals and
the beam driver."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests import stress_np as snp
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_gpu, perturbed_state
from tests.test_stress import ATOL, EPS, G, H_STEP, Q_ROT, SOFT, gravity_run, moduli

tl = importlib.import_module("total-lagrangian-fea_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
SIGMA = {"cube": 1e-3, "res2": 1e-3, "bunny": 1e-4}


def move(d, x):
    d.UpdatePositions(x[:, 0], x[:, 1], x[:, 2])


def gpu_restated(d, m, v=None, ids=None, materials=None):
    """The restatement on the GPU's own F, det J and connectivity (existing retrieve calls)."""
    d.CalcP()
    F = d.RetrieveDeformationGradientToCPU()
    conn = d.RetrieveConnectivityToCPU()
    Fd = snp.deformation(v.reshape(-1, 3), conn, d.RetrieveDnDuPreToCPU()) if v is not None else None
    return snp.recover(F, m if ids is None else ids, d.RetrieveDetJToCPU(), tl.quadrature.tet5pt_weights, conn,
                       d.get_n_coef(), Fd, materials)


def fields(d, points=True):
    e, n, t = d.RetrieveElementStressToCPU(), d.RetrieveNodalStressToCPU(), d.GetEnergies()
    out = dict(elem_sigma=e.sigma, elem_von_mises=e.von_mises, elem_psi=e.psi, elem_J=e.J, elem_volume=e.volume,
               nodal_sigma=n.sigma, nodal_von_mises=n.von_mises, strain_energy=t.strain, kinetic=t.kinetic,
               viscous_power=t.viscous_power, reference_volume=t.reference_volume, current_volume=t.current_volume)
    if points:
        out["point_sigma"] = d.RetrievePointStressToCPU()
    return out


FIELDS = ("point_sigma", "elem_sigma", "elem_von_mises", "elem_psi", "elem_J", "elem_volume", "nodal_sigma", "nodal_von_mises")
TOTALS = ("strain_energy", "viscous_power", "reference_volume", "current_volume")


# ---- 1. parity with the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_v", [False, True])
@pytest.mark.parametrize("mat", ["svk", "mr", "neo", "mr_damped"])
@pytest.mark.parametrize("tag", ["res2", "bunny"])
def test_parity_with_restatement(tag, mat, with_v):
    X, conn = load_mesh(tag)
    m = MATERIALS[mat]
    x, v = perturbed_state(X, sigma=SIGMA[tag])
    d = make_gpu(X, conn, m)
    move(d, x)
    ref = gpu_restated(d, m, v if with_v else None)
    d.CalcStress(v if with_v else None, points=True)
    got = fields(d)
    for name in FIELDS:
        scale = np.abs(ref[name]).max()
        err = np.abs(got[name] - ref[name]).max()
        print(f"{tag} {mat} v={with_v} {name}: {err / scale:.2e}")
        assert err <= 1e-10 * scale, name
    # The strain-energy densities are differences of O(modulus) terms (Mooney-Rivlin: mu10 (J^-2/3 I1 - 3), kappa/2 (J-1)^2
    # from J ~ 1), so each carries a few ulp of the moduli whatever the strain: the floor of tests/test_oracle_mr.py,
    # 256 eps x the sum of moduli, integrated over the volume, stands next to the 1e-12 of the total (bunny,
    # Mooney-Rivlin, 6e-12 of a 4.8e4 J total at strains of 1e-3, against a floor of this size).
    floor = {"strain_energy": 256 * EPS * moduli(m) * ref["reference_volume"]}
    for name in TOTALS:
        err = abs(got[name] - ref[name])
        print(f"{tag} {mat} v={with_v} {name}: {got[name]:.15e} vs {ref[name]:.15e}")
        assert err <= 1e-12 * abs(ref[name]) + floor.get(name, 0.0), name
    if with_v:
        off, col, val = d.RetrieveMassCSRToCPU()
        ke = snp.kinetic_energy(off, col, val, v)
        assert abs(got["kinetic"] - ke) <= 1e-12 * ke
        if m["eta"] != 0:
            assert got["viscous_power"] > 0
    else:
        assert got["kinetic"] == 0.0 and got["viscous_power"] == 0.0
    d.Destroy()


# ---- 2. force-stress identity on the device path -----------------------------------------------------------------------
@pytest.mark.parametrize("mat", ["svk", "mr", "neo"])
@pytest.mark.parametrize("tag", ["res2", "bunny"])
def test_force_stress_identity(tag, mat):
    """sum_q sigma J dV = sum_a f_int,a (x) x_a with f_int from the oracle-pinned force path: no restatement between."""
    X, conn = load_mesh(tag)
    x, _ = perturbed_state(X, sigma=SIGMA[tag])
    d = make_gpu(X, conn, MATERIALS[mat])
    move(d, x)
    d.CalcP()
    d.CalcInternalForce()
    f = d.RetrieveInternalForceToCPU().reshape(-1, 3)
    J = np.linalg.det(d.RetrieveDeformationGradientToCPU())
    d.CalcStress(points=True)
    sig = snp.tensor(d.RetrievePointStressToCPU())
    dV = d.RetrieveDetJToCPU() * tl.quadrature.tet5pt_weights[None, :]
    lhs = np.einsum("eq,eqij->ij", J * dV, sig)
    rhs = np.einsum("ai,aj->ij", f, x)
    err = np.abs(lhs - rhs).max() / np.abs(rhs).max()
    print(f"{tag} {mat}: {err:.2e}")
    assert err <= 1e-10
    d.Destroy()


# ---- 3. homogeneous deformation, rigid rotation ------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(G["F"])))
def test_homogeneous_deformation(k):
    F0, (mu10, mu01, kappa), P_ref = G["F"][k], G["params"][k], G["P"][k]
    m = dict(kind="mr", mu10=mu10, mu01=mu01, kappa=kappa, rho0=1000.0, eta=0.0, lamd=0.0)
    X, conn = load_mesh("cube")
    d = make_gpu(X, conn, m)
    move(d, X @ F0.T)
    d.CalcStress(points=True)
    got = fields(d)
    s_ref = snp.voigt(P_ref @ F0.T / np.linalg.det(F0))
    tol = 1e-12 * np.abs(s_ref).max() + 256 * EPS * (kappa + mu10 + mu01)
    for name in ("point_sigma", "elem_sigma", "nodal_sigma"):
        assert np.abs(got[name] - s_ref).max() <= tol, name
    assert np.abs(got["nodal_von_mises"] - snp.von_mises(s_ref)).max() <= 2 * tol
    assert abs(got["current_volume"] - np.linalg.det(F0) * got["reference_volume"]) <= 1e-12 * got["reference_volume"]
    d.Destroy()


@pytest.mark.parametrize("mat", ["svk", "mr"])
def test_objectivity(mat):
    X, conn = load_mesh("res2")
    m = MATERIALS[mat]
    x, _ = perturbed_state(X, sigma=1e-3)
    d = make_gpu(X, conn, m)
    out = []
    for xx in (x, x @ Q_ROT.T, X @ Q_ROT.T):
        move(d, xx)
        d.CalcStress(points=True)
        out.append(fields(d))
    a, b, rigid = out
    scale = np.abs(a["point_sigma"]).max()
    rot = snp.voigt(Q_ROT @ snp.tensor(a["point_sigma"]) @ Q_ROT.T)
    assert np.abs(b["point_sigma"] - rot).max() <= 1e-10 * scale + 256 * EPS * moduli(m)
    for name in ("elem_von_mises", "nodal_von_mises", "elem_psi"):
        assert np.abs(a[name] - b[name]).max() <= 1e-10 * np.abs(a[name]).max() + 256 * EPS * moduli(m), name
    for name in ("strain_energy", "reference_volume", "current_volume"):
        assert abs(a[name] - b[name]) <= 1e-10 * abs(a[name]), name
    assert np.abs(rigid["point_sigma"]).max() <= 1e-9 * moduli(m)
    assert np.abs(rigid["nodal_von_mises"]).max() <= 1e-9 * moduli(m)
    d.Destroy()


# ---- 4. per-element materials ------------------------------------------------------------------------------------------
def test_per_element_materials():
    X, conn = load_mesh("cube")
    n, E = X.shape[0], conn.shape[0]
    F0 = G["F"][4]                                              # a 10 % stretch with shear (not the identity of entry 0)
    stiff = dict(kind="svk", E=7e8, nu=0.33, rho0=2700.0, eta=0.0, lamd=0.0)
    soft = dict(kind="svk", E=2e6, nu=0.45, rho0=900.0, eta=0.0, lamd=0.0)
    single = []
    for m in (stiff, soft):
        d = make_gpu(X, conn, m)
        move(d, X @ F0.T)
        d.CalcStress(points=True)
        single.append(fields(d))
        d.Destroy()
    X2, conn2 = np.vstack([X, X + np.array([0.0, 5.0, 0.0])]), np.vstack([conn, conn + n])
    ids = np.repeat([0, 1], E).astype(np.int32)
    entries = [tl.ElementMaterial(E=m["E"], nu=m["nu"], rho0=m["rho0"]) for m in (stiff, soft)]
    d = make_gpu(X2, conn2, stiff)
    move(d, np.vstack([X @ F0.T, (X + np.array([0.0, 5.0, 0.0])) @ F0.T]))
    d.CalcStress(points=True)
    before = fields(d)
    d.SetElementMaterials(ids, entries, "svk")
    d.CalcStress(points=True)                                   # the new table is used at once
    got = fields(d)
    assert np.allclose(before["elem_sigma"][:E], got["elem_sigma"][:E], rtol=1e-13, atol=0)
    assert not np.allclose(before["elem_sigma"][E:], got["elem_sigma"][E:])
    for b, (es, ns) in enumerate(((slice(0, E), slice(0, n)), (slice(E, 2 * E), slice(n, 2 * n)))):
        for name in FIELDS:
            sel = ns if name.startswith("nodal") else es
            scale = np.abs(single[b][name]).max()
            assert np.abs(got[name][sel] - single[b][name]).max() <= 1e-13 * scale, (b, name)
    assert abs(got["strain_energy"] - single[0]["strain_energy"] - single[1]["strain_energy"]) <= 1e-13 * got["strain_energy"]
    d.Destroy()


# ---- 5. with a solver --------------------------------------------------------------------------------------------------
def cantilever(tag="res4"):
    X, conn = load_mesh(tag)
    d = make_gpu(X, conn, SOFT, fixed_x0(X))
    off, col, val = d.RetrieveMassCSRToCPU()
    mass = np.add.reduceat(val, off[:-1])
    d.SetExternalForce((mass[:, None] * np.array([0.0, 0.0, -9.81])[None, :]).reshape(-1))
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.SetParameters(tl.SyncedNewtonParams(ATOL, 0.0, 1e-6, 1e14, 1, 40, H_STEP))
    s.SetLinSolveOpts(tl.LinSolveOpts(rel_tol=1e-13, max_iter=50000))
    return X, d, s, mass, (off, col, val)


def test_energies_with_a_solver():
    X, d, s, mass, (off, col, val) = cantilever()

    def positions():
        return np.stack(d.RetrievePositionToCPU(), axis=1)

    def energies():
        d.CalcStress(s)
        t = d.GetEnergies()
        ke = snp.kinetic_energy(off, col, val, s.RetrieveVelocityToCPU())
        assert abs(t.kinetic - ke) <= 1e-12 * ke
        assert t.strain > 0
        return t.strain, t.kinetic

    tot, bound = gravity_run(s.Solve, X, mass, H_STEP, 20, energies, positions)
    growth = np.diff(tot)
    print("energy growth per step / bound:", np.max(growth / bound), "total", tot[-1])
    assert np.all(growth <= bound)      # confirmed on the oracle path by tests/test_stress.py
    assert tot[-1] < 0
    del s
    d.Destroy()


# ---- 6. does not disturb a step ----------------------------------------------------------------------------------------
def test_does_not_disturb_a_step():
    out = []
    for with_stress in (False, True):
        X, d, s, _, _ = cantilever("res2")
        for _ in range(3):
            s.Solve()
            if with_stress:
                d.CalcStress(s, points=True)
        out.append((np.stack(d.RetrievePositionToCPU()), s.RetrieveVelocityToCPU()))
        del s
        d.Destroy()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 7. determinism ----------------------------------------------------------------------------------------------------
def test_determinism():
    X, conn = load_mesh("bunny")
    m = MATERIALS["mr_damped"]
    x, v = perturbed_state(X, sigma=1e-4)
    runs = []
    for _ in range(2):
        d = make_gpu(X, conn, m)
        move(d, x)
        for _ in range(2):
            d.CalcStress(v, points=True)
            f = fields(d)
            runs.append([f[k] for k in sorted(f)])
        d.Destroy()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    X, conn = load_mesh("beam_3x2x1")
    q = tl.quadrature
    d = tl.GPU_FEAT10_Data(conn.shape[0], X.shape[0])
    d.Initialize()
    d.Setup(q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights, X[:, 0], X[:, 1], X[:, 2], conn)
    d.SetDensity(1000.0)
    d.SetSVK(1e7, 0.3)
    with pytest.raises(tl.TlfeaError, match="CalcDnDuPre"):
        d.CalcStress()
    d.CalcDnDuPre()
    for call in (d.RetrieveElementStressToCPU, d.RetrieveNodalStressToCPU, d.RetrievePointStressToCPU, d.GetEnergies):
        with pytest.raises(tl.TlfeaError, match="has not been called"):
            call()
    with pytest.raises(tl.TlfeaError, match="CalcMassMatrix"):
        d.CalcStress(np.zeros(3 * X.shape[0]))
    d.CalcStress()                                              # works without a mass matrix or a solver
    assert d.GetEnergies().reference_volume == pytest.approx(6.0, rel=1e-12)
    with pytest.raises(tl.TlfeaError, match="point stresses"):
        d.RetrievePointStressToCPU()
    with pytest.raises(ValueError, match="entries"):
        d.CalcStress(np.zeros(5))
    d.Destroy()
    a = tl.GPU_ANCF3243_Data(2, 1)
    a.Initialize()
    with pytest.raises(tl.TlfeaError, match="ANCF"):
        a.CalcStress()
    with pytest.raises(tl.TlfeaError, match="ANCF"):
        a.RetrieveNodalStressToCPU()
    a.Destroy()


# ---- 9. driver ---------------------------------------------------------------------------------------------------------
def test_beam_stress_driver(tmp_path):
    exe = os.path.join(HOST, "test_beam_stress")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    vtu = tmp_path / "beam_stress.vtu"
    p = subprocess.run(["timeout", "-k", "10", "300", exe, "--mesh_dir=" + os.path.join(ROOT, "tests", "golden", "meshes"),
                        "--res=2", "--steps=5", "--vtu=" + str(vtu)], capture_output=True, text=True, timeout=320)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("Step")]) == 5
    txt = vtu.read_text()
    n = int(re.search(r'NumberOfPoints="(\d+)"', txt).group(1))
    for name, comps in (("displacement", 3), ("stress", 6), ("von_mises", 1)):
        body = re.search(r'<DataArray type="Float64" Name="%s"[^>]*>\n(.*?)</DataArray>' % name, txt, re.S).group(1)
        rows = [ln for ln in body.splitlines() if ln.strip()]
        assert len(rows) == n and all(len(r.split()) == comps for r in rows), name
