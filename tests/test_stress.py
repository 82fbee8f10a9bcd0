"""Stress recovery without a GPU: the NumPy restatement tests/stress_np.py is pinned to the oracle (itself
pinned to the reference's vectors) -- stress against the oracle's P, the discrete force-stress identity, the energy whose
derivative is the internal force, homogeneous deformation against the symbolic golden P, objectivity, the kinetic energy --
so that the GPU tests do not compare the kernels with a twin of themselves.  Also: the energy balance of backward Euler on
the oracle path that tests/test_gpu_stress.py asserts on the GPU, and the exported symbols."""
import os

import numpy as np
import pytest

from oracle import orc
from tests import stress_np as snp
from tests.helpers import MATERIALS, fixed_x0, load_mesh, make_oracle, perturbed_state, tl

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "mr_energy_derivatives.npz"))
EPS = np.finfo(float).eps
SIGMA = {"cube": 1e-3, "res2": 1e-3, "bunny": 1e-4}
Q_ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])   # proper rotation (exact in decimals)
NEW = ("tlfea_t10_calc_stress", "tlfea_t10_calc_stress_host", "tlfea_t10_retrieve_point_stress",
       "tlfea_t10_retrieve_element_stress", "tlfea_t10_retrieve_nodal_stress", "tlfea_t10_get_energies",
       "tlfea_t10_nodal_stress_device_ptr", "tlfea_t10_time_stress_kernels")


def moduli(m):
    return sum(snp.lame(m)) if m["kind"] == "svk" else m["kappa"] + m["mu10"] + m["mu01"]


def mats33(A):
    """(E, 5, 9) column-major 3x3 buffers of the oracle -> [E, 5, 3, 3]."""
    return A.reshape(A.shape[0], 5, 3, 3).transpose(0, 1, 3, 2)


def state(tag, mat):
    X, conn = load_mesh(tag)
    m = MATERIALS[mat]
    o = make_oracle(X, conn, m)
    x, v = perturbed_state(X, sigma=SIGMA[tag])
    o.x, o.y, o.z = (np.ascontiguousarray(x[:, c]) for c in range(3))
    return X, conn, m, o, x, v


def restated(o, m, x, conn, v=None):
    g = o.gradN_a_d()
    F = snp.deformation(x, conn, g)
    Fd = snp.deformation(v.reshape(-1, 3), conn, g) if v is not None else None
    return snp.recover(F, m, o.detJ, o.qw, conn, x.shape[0], Fd)


@pytest.mark.parametrize("mat", ["svk", "mr", "svk_damped"])
@pytest.mark.parametrize("tag", ["cube", "res2", "bunny"])
def test_stress_against_oracle(tag, mat):
    X, conn, m, o, x, v = state(tag, mat)
    r = restated(o, m, x, conn, v)
    assert r["J"].min() > 0.9
    _, P, _, _ = o.compute_p(v)
    P = mats33(P)
    # sigma J F^-T back to P: the restated Cauchy stress carries the oracle's first Piola-Kirchhoff stress
    F = snp.deformation(x, conn, o.gradN_a_d())
    back = r["J"][..., None, None] * r["point_sigma_full"] @ np.swapaxes(np.linalg.inv(F), -1, -2)
    err = np.abs(back - P).max()
    print(f"{tag} {mat}: max |sigma J F^-T - P| = {err:.3e}, max |P| = {np.abs(P).max():.3e}")
    assert err <= 1e-12 * np.abs(P).max() + 256 * EPS * moduli(m)
    assert np.abs(r["point_sigma_full"] - np.swapaxes(r["point_sigma_full"], -1, -2)).max() <= 1e-12 * np.abs(P).max() + 256 * EPS * moduli(m)


@pytest.mark.parametrize("mat", ["svk", "mr", "svk_damped"])
@pytest.mark.parametrize("tag", ["cube", "res2", "bunny"])
def test_force_stress_identity(tag, mat):
    """sum_q sigma J dV = sum_a f_int,a (x) x_a: exact in the discrete setting at any configuration."""
    X, conn, m, o, x, v = state(tag, mat)
    r = restated(o, m, x, conn, v)
    dV = o.detJ * o.qw[None, :]
    lhs = np.einsum("eq,eqij->ij", r["J"] * dV, r["point_sigma_full"])
    rhs = np.einsum("ai,aj->ij", o.internal_force(v).reshape(-1, 3), x)
    err = np.abs(lhs - rhs).max() / np.abs(rhs).max()
    print(f"{tag} {mat}: force-stress identity {err:.3e}")
    assert err <= 1e-10
    assert np.abs(rhs - rhs.T).max() <= 1e-10 * np.abs(rhs).max()


@pytest.mark.parametrize("mat", ["svk", "mr"])
def test_energy_derivative(mat):
    """central difference of the restated strain energy along a unit direction = f_int . d"""
    X, conn, m, o, x, _ = state("res2", mat)
    d = np.random.default_rng(1).normal(size=x.shape)
    d /= np.linalg.norm(d)
    delta = 1e-5 * np.ptp(X, axis=0).max()
    Wp = restated(o, m, x + delta * d, conn)["strain_energy"]
    Wm = restated(o, m, x - delta * d, conn)["strain_energy"]
    fd = (Wp - Wm) / (2 * delta)
    ref = float(o.internal_force(None) @ d.reshape(-1))
    print(f"{mat}: dW/dd = {fd:.9e}, f_int.d = {ref:.9e}, relative difference {abs(fd - ref) / abs(ref):.2e}")
    assert abs(fd - ref) <= 1e-6 * abs(ref)


@pytest.mark.parametrize("k", range(len(G["F"])))
def test_homogeneous_deformation(k):
    F0, (mu10, mu01, kappa), P_ref = G["F"][k], G["params"][k], G["P"][k]
    m = dict(kind="mr", mu10=mu10, mu01=mu01, kappa=kappa, rho0=1000.0, eta=0.0, lamd=0.0)
    X, conn = load_mesh("cube")
    o = make_oracle(X, conn, m)
    x = X @ F0.T
    r = restated(o, m, x, conn)
    s_ref = snp.voigt(P_ref @ F0.T / np.linalg.det(F0))
    tol = 1e-12 * np.abs(s_ref).max() + 256 * EPS * (kappa + mu10 + mu01)
    for name in ("point_sigma", "elem_sigma", "nodal_sigma"):
        assert np.abs(r[name] - s_ref).max() <= tol, name
    assert abs(r["current_volume"] - np.linalg.det(F0) * r["reference_volume"]) <= 1e-12 * r["reference_volume"]
    assert abs(r["reference_volume"] - (o.detJ * o.qw).sum()) <= 1e-14


@pytest.mark.parametrize("mat", ["svk", "mr"])
def test_objectivity(mat):
    X, conn, m, o, x, _ = state("res2", mat)
    assert np.allclose(Q_ROT @ Q_ROT.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(Q_ROT) - 1) < 1e-15
    a, b = restated(o, m, x, conn), restated(o, m, x @ Q_ROT.T, conn)
    scale = np.abs(a["point_sigma"]).max()
    rot = snp.voigt(Q_ROT @ a["point_sigma_full"] @ Q_ROT.T)
    assert np.abs(b["point_sigma"] - rot).max() <= 1e-10 * scale + 256 * EPS * moduli(m)
    for name in ("elem_von_mises", "nodal_von_mises", "elem_psi"):
        assert np.abs(a[name] - b[name]).max() <= 1e-10 * np.abs(a[name]).max() + 256 * EPS * moduli(m), name
    for name in ("strain_energy", "reference_volume", "current_volume"):
        assert abs(a[name] - b[name]) <= 1e-10 * abs(a[name]), name
    rigid = restated(o, m, X @ Q_ROT.T, conn)
    assert np.abs(rigid["point_sigma"]).max() <= 1e-9 * moduli(m)
    assert abs(rigid["strain_energy"]) <= 1e-9 * moduli(m) * rigid["reference_volume"]


def test_kinetic_energy():
    X, conn, m, o, x, v = state("res2", "svk")
    n = X.shape[0]
    M = np.zeros((n, n))
    for i in range(n):
        M[i, o.m_col[o.m_off[i]:o.m_off[i + 1]]] = o.m_val[o.m_off[i]:o.m_off[i + 1]]
    v3 = v.reshape(-1, 3)
    ref = 0.5 * sum(v3[:, c] @ M @ v3[:, c] for c in range(3))
    assert abs(snp.kinetic_energy(o.m_off, o.m_col, o.m_val, v) - ref) <= 1e-13 * ref
    assert abs(M.sum() - m["rho0"] * (o.detJ * o.qw).sum()) <= 1e-10 * M.sum()


def gravity_run(step, X, mass, h, steps, energies, positions):
    """Total of strain, kinetic and gravity energy after each step of a cantilever falling from rest, and the bound on
    its growth.  Backward Euler solved exactly only loses energy; a step left with a residual ||g|| <= atol (force units)
    can gain at most g . (x_new - x_old) <= atol ||x_new - x_old||, plus the round-off of the three sums."""
    f_ext = (mass[:, None] * np.array([0.0, 0.0, -9.81])[None, :]).reshape(-1)
    tot, bound = [0.0], []
    x_old = X.copy()
    for _ in range(steps):
        step()
        x = positions()
        W, K = energies()
        U = -float(f_ext @ (x - X).reshape(-1))
        tot.append(W + K + U)
        bound.append(ATOL * np.linalg.norm(x - x_old) + 64 * EPS * (abs(W) + abs(K) + abs(U)))
        x_old = x
    return np.array(tot), np.array(bound)


ATOL, H_STEP, SOFT = 1e-7, 0.05, dict(kind="svk", E=1e7, nu=0.3, rho0=1000.0, eta=0.0, lamd=0.0)


def test_backward_euler_does_not_gain_energy_on_the_oracle():
    X, conn = load_mesh("res2")
    o = make_oracle(X, conn, SOFT, fixed_x0(X))
    mass = np.add.reduceat(o.m_val, o.m_off[:-1])
    o.f_ext = (mass[:, None] * np.array([0.0, 0.0, -9.81])[None, :]).reshape(-1).copy()
    prm = orc.NewtonParams(ATOL, 0.0, 1e-6, 1e14, 1, 40, H_STEP)

    def positions():
        return np.stack([o.x, o.y, o.z], axis=1)

    def energies():
        r = restated(o, SOFT, positions(), conn)
        return r["strain_energy"], snp.kinetic_energy(o.m_off, o.m_col, o.m_val, o.v)

    tot, bound = gravity_run(lambda: o.newton_step(prm, solver=0), X, mass, H_STEP, 20, energies, positions)
    growth = np.diff(tot)
    print("oracle energy growth per step / bound:", np.max(growth / bound), "total", tot[-1])
    assert np.all(growth <= bound)
    assert tot[-1] < 0


def test_symbols_exported():
    syms = tl.exported_symbols()
    assert all(s in syms for s in NEW)
    lib = tl.load_library()
    assert all(hasattr(lib, s) for s in NEW)
    for name in ("CalcStress", "RetrievePointStressToCPU", "RetrieveElementStressToCPU", "RetrieveNodalStressToCPU",
                 "GetEnergies"):
        assert hasattr(tl.GPU_FEAT10_Data, name)
