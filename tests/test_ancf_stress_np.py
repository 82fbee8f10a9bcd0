"""The NumPy restatement tests/ancf_stress_np.py of the ANCF stress recovery (DESIGN 3f'), pinned without a GPU so that
tests/test_gpu_ancf_stress.py compares the kernels with something already checked.  ANCF represents affine maps exactly
(positions A X, gradient coefficients A e_i), which gives closed-form answers; the oracle's own F and P pin the rest."""
import numpy as np
import pytest

from tests import ancf_stress_np as anp
from tests import stress_np as snp
from tests.helpers import MATERIALS, tl

EPS = np.finfo(float).eps
PROBLEMS = {"beam2": lambda: anp.beam_line(2), "plate2x2": lambda: anp.shell_plate(2, 2)}
NEW = ("tlfea_ancf_calc_stress", "tlfea_ancf_calc_stress_host", "tlfea_ancf_retrieve_point_stress",
       "tlfea_ancf_retrieve_element_stress", "tlfea_ancf_retrieve_nodal_stress", "tlfea_ancf_get_energies",
       "tlfea_ancf_nodal_stress_device_ptr", "tlfea_ancf_time_stress_kernels")


def volume(prob):
    L, W, H = prob[5]
    return prob[4].shape[0] * L * W * H


@pytest.mark.parametrize("mat", ["svk", "mr"])
@pytest.mark.parametrize("pname", sorted(PROBLEMS))
def test_affine_map(pname, mat):
    prob, m, A = PROBLEMS[pname](), MATERIALS[mat], anp.A_STRETCH
    o = anp.make_oracle(prob, m)
    r = anp.recover(o, m, anp.coefficients(o) @ A.T)
    assert np.abs(r["F"] - A).max() <= 64 * EPS                     # every point's F is A
    s_ref = anp.cauchy_closed_form(A, m)
    tol = 1e-12 * np.abs(s_ref).max() + 256 * EPS * anp.moduli(m)
    for name in ("point_sigma", "elem_sigma", "nodal_sigma"):
        assert np.abs(r[name] - s_ref).max() <= tol, name
    assert np.abs(r["nodal_von_mises"] - snp.von_mises(s_ref)).max() <= 2 * tol
    V = volume(prob)
    assert abs(r["reference_volume"] - V) <= 1e-12 * V
    assert abs(r["current_volume"] - np.linalg.det(A) * V) <= 1e-12 * V
    W = float(snp.psi(A, m)) * V
    assert abs(r["strain_energy"] - W) <= 1e-12 * W + 256 * EPS * anp.moduli(m) * V
    assert np.abs(r["elem_J"] - np.linalg.det(A)).max() <= 1e-12
    assert np.abs(r["elem_volume"].sum() - V) <= 1e-12 * V


@pytest.mark.parametrize("mat", ["svk", "mr"])
@pytest.mark.parametrize("pname", sorted(PROBLEMS))
def test_rigid_rotation(pname, mat):
    prob, m = PROBLEMS[pname](), MATERIALS[mat]
    o = anp.make_oracle(prob, m)
    r = anp.recover(o, m, anp.coefficients(o) @ anp.Q_ROT.T + np.array([0.3, -0.2, 0.1]) * (np.arange(o.N) % 4 == 0)[:, None])
    K = anp.moduli(m)
    assert np.abs(r["point_sigma"]).max() <= 1e-12 * K
    assert np.abs(r["nodal_von_mises"]).max() <= 1e-12 * K
    assert abs(r["strain_energy"]) <= 1e-12 * K * volume(prob)
    assert abs(r["current_volume"] - r["reference_volume"]) <= 1e-12 * r["reference_volume"]


@pytest.mark.parametrize("mat", ["svk", "mr", "svk_damped", "mr_damped"])
@pytest.mark.parametrize("pname", sorted(PROBLEMS))
def test_against_the_oracle(pname, mat):
    """F and the residual's P (elastic + Kelvin-Voigt) of the oracle at a perturbed state; the force-stress identity
    sum_q sigma J dV = sum_a f_int,a (x) x_a; the kinetic energy against the dense mass matrix."""
    prob, m = PROBLEMS[pname](), MATERIALS[mat]
    o = anp.make_oracle(prob, m)
    x, v = anp.perturbed(o)
    anp.set_state(o, x)
    r = anp.recover(o, m, x, v)
    assert r["J"].min() > 0.9
    F, P = (a.reshape(o.E, o.Q, 3, 3).transpose(0, 1, 3, 2) for a in o.compute_p(v))   # column-major 3 x 3 buffers
    assert np.abs(r["F"] - F).max() <= 1e-13 * np.abs(F).max()
    back = r["J"][..., None, None] * r["point_sigma_full"] @ np.swapaxes(np.linalg.inv(r["F"]), -1, -2)
    assert np.abs(back - P).max() <= 1e-12 * np.abs(P).max() + 256 * EPS * anp.moduli(m)
    dV = o.detJ * o.qw[None, :]
    lhs = np.einsum("eq,eqij->ij", r["J"] * dV, r["point_sigma_full"])
    rhs = np.einsum("ai,aj->ij", o.internal_force(v).reshape(-1, 3), x)
    assert np.abs(lhs - rhs).max() <= 1e-10 * np.abs(rhs).max()
    v3 = v.reshape(-1, 3)
    ke = 0.5 * np.einsum("ai,ab,bi->", v3, o.mass_dense(), v3)
    assert abs(r["kinetic"] - ke) <= 1e-12 * ke
    if m["eta"] != 0:
        assert r["viscous_power"] > 0
    else:
        assert r["viscous_power"] == 0.0


def test_node_average_by_hand():
    """2 x 2 plate: the centre node averages all four shells, a corner node has its one shell's mean, in Voigt order."""
    prob, m = PROBLEMS["plate2x2"](), MATERIALS["svk"]
    o = anp.make_oracle(prob, m)
    x, _ = anp.perturbed(o)
    r = anp.recover(o, m, x)
    assert r["nodal_sigma"].shape == (9, 6)
    w = r["elem_volume"]
    centre = (w[:, None] * r["elem_sigma"]).sum(axis=0) / w.sum()
    assert np.abs(r["nodal_sigma"][4] - centre).max() <= 1e-13 * np.abs(centre).max()
    assert np.array_equal(r["nodal_sigma"][0], r["elem_sigma"][0] * w[0] / w[0])
    assert np.abs(r["nodal_von_mises"] - snp.von_mises(r["nodal_sigma"])).max() == 0.0


@pytest.mark.parametrize("mat", ["svk", "mr"])
@pytest.mark.parametrize("pname", sorted(PROBLEMS))
def test_strain_energy_derivative_is_the_internal_force(pname, mat):
    """Central difference of the restated strain energy along a random direction against the oracle's f_int . dx, the
    check tests/test_gpu_ancf_stress.py repeats through the GPU with this one's error x 10 as its bound.  What is left at
    a step eps is the truncation of the central difference, c eps^2: halving eps divides it by 4 (found: 4.00 +- 0.01 on
    both meshes and both materials from eps = 4e-4 down to 5e-5, the error at 1e-4 being 3e-7 .. 9e-6 of f . dx), which no
    wrong energy or wrong force would do, and which shows that rounding is far below the truncation at FD_EPS."""
    prob, m = PROBLEMS[pname](), MATERIALS[mat]
    o = anp.make_oracle(prob, m)
    x, _ = anp.perturbed(o)

    def force(xx):
        anp.set_state(o, xx)
        return o.internal_force(None)

    err = []
    for eps in (2 * anp.FD_EPS, anp.FD_EPS):
        fd, fdx, _ = anp.energy_fd(lambda xx: anp.recover(o, m, xx)["strain_energy"], force, x, eps)
        err.append(abs(fd - fdx) / abs(fdx))
    print(f"{pname} {mat}: relative error {err[0]:.3e} at 2 eps, {err[1]:.3e} at eps, ratio {err[0] / err[1]:.3f}")
    assert 3.9 <= err[0] / err[1] <= 4.1
    assert err[1] <= 1e-4            # eps^2 (1e-8) x the curvature ratio of a state strained by 1e-3 .. 1e-2


def test_symbols_and_members():
    syms = tl.exported_symbols()
    assert all(s in syms for s in NEW)
    lib = tl.load_library()
    assert all(hasattr(lib, s) for s in NEW)
    for cls in (tl.GPU_ANCF3243_Data, tl.GPU_ANCF3443_Data):
        for name in ("CalcElementStress", "RetrieveANCFPointStressToCPU", "RetrieveANCFElementStressToCPU",
                     "RetrieveANCFNodalStressToCPU", "GetANCFEnergies", "TimeANCFStressKernels"):
            assert hasattr(cls, name)
