"""NumPy restatement of the stress recovery of the ANCF kinds (DESIGN 3f'): F per (element, point) from an AncfOracle after
calc_dsdu_pre, the constitutive pieces of tests/stress_np.py, and the means, the mesh-node average (node = coefficient // 4,
ascending elements) and the totals in plain NumPy.  Also the meshes the two test files share."""
import numpy as np

from oracle import orc
from tests import stress_np as snp
from tests.helpers import oracle_material, tl

mu = tl.mesh_utils
BEAM_DIMS = (0.5, 0.1, 0.1)     # L, W, H of the beam problems of tests/test_gpu_ancf.py
SHELL_DIMS = (2.0, 1.0, 0.1)


def beam_line(n_elem):
    """n_elem ANCF-3243 beams on one line -> (kind, x12, y12, z12, conn_nodes, (L, W, H))"""
    L = BEAM_DIMS[0]
    gen = mu.GridMeshGenerator(n_elem * L, 0.0, L, True, False)
    gen.generate_mesh()
    return (3243,) + gen.get_coordinates() + (gen.get_element_connectivity(), BEAM_DIMS)


def shell_plate(nx, ny):
    """nx x ny ANCF-3443 shells (2 x 2: the centre node belongs to four of them)"""
    return (3443,) + mu.structured_3443_plate(nx, ny, SHELL_DIMS[0], SHELL_DIMS[1]) + (SHELL_DIMS,)


def net(path):
    """a `.ancf3243mesh` net (W = H = 0.1 as its driver); its constraint rows play no part in the stress recovery"""
    m = mu.ReadANCF3243MeshFromFile(path)
    return 3243, m.x12, m.y12, m.z12, m.element_connectivity, (m.grid_L, 0.1, 0.1)


def make_oracle(prob, m):
    kind, x, y, z, conn, (L, W, H) = prob
    o = orc.AncfOracle(kind, x, y, z, conn, L, W, H, oracle_material(m))
    o.calc_dsdu_pre()
    o.calc_mass()
    return o


def coefficients(o):
    """[n_coef, 3] reference coefficient vectors (positions and gradients) of the oracle"""
    return np.stack([o.xt, o.yt, o.zt], axis=1)


def deformation(o, c):
    """F [E, Q, 3, 3] = sum_a c_a (x) grad s_a for coefficient vectors c [n_coef, 3] (positions, or velocities for Fdot)"""
    return np.einsum("eai,eqja->eqij", np.asarray(c)[o.conn], o.gradN)


def recover(o, m, x, v=None):
    """Every field and total of tlfea_ancf_calc_stress at the coefficients x [n_coef, 3] (velocity v [3 n_coef] or None)."""
    F = deformation(o, x)
    Fd = deformation(o, np.asarray(v).reshape(-1, 3)) if v is not None else None
    damped = Fd is not None and (m["eta"] != 0 or m["lamd"] != 0)
    P = snp.elastic_P(F, m)
    Pv = snp.viscous_P(F, Fd, m) if damped else np.zeros_like(F)
    W = snp.psi(F, m)
    J = np.linalg.det(F)
    sig_full = (P + Pv) @ np.swapaxes(F, -1, -2) / J[..., None, None]
    sig = snp.voigt(sig_full)
    power = np.sum(Pv * Fd, axis=(-2, -1)) if damped else np.zeros(F.shape[:2])
    dV = o.detJ * o.qw[None, :]
    Ve = dV.sum(axis=1)
    wq = dV / Ve[:, None]
    es = np.einsum("eq,eqc->ec", wq, sig)
    n_nodes = o.N // 4
    node_conn = o.conn[:, 0::4] // 4                       # slot 0 of every local node
    num, den = np.zeros((n_nodes, 6)), np.zeros(n_nodes)
    for e in range(o.E):                                   # ascending elements
        for n in node_conn[e]:
            num[n] += Ve[e] * es[e]
            den[n] += Ve[e]
    ns = num / np.where(den > 0, den, 1.0)[:, None]
    kinetic = snp.kinetic_energy(o.m_off, o.m_col, o.m_val, v) if v is not None else 0.0
    return dict(F=F, P=P + Pv, J=J, point_sigma=sig, point_sigma_full=sig_full, elem_sigma=es,
                elem_von_mises=snp.von_mises(es), elem_psi=(wq * W).sum(axis=1), elem_J=(wq * J).sum(axis=1),
                elem_volume=Ve, nodal_sigma=ns, nodal_von_mises=snp.von_mises(ns), strain_energy=float((W * dV).sum()),
                kinetic=kinetic, viscous_power=float((power * dV).sum()), reference_volume=float(dV.sum()),
                current_volume=float((J * dV).sum()))


# ---- known answers ---------------------------------------------------------------------------------------------------
A_STRETCH = np.array([[1.10, 0.04, 0.00], [0.02, 0.95, 0.03], [0.00, -0.05, 1.05]])   # stretch with shear, det > 0
Q_ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])           # proper rotation (exact in decimals)


def second_pk(A, m):
    """Closed-form second Piola-Kirchhoff stress S(A), written independently of stress_np.elastic_P"""
    C = A.T @ A
    if m["kind"] == "svk":
        lam, mu_ = snp.lame(m)
        E = 0.5 * (C - np.eye(3))
        return lam * np.trace(E) * np.eye(3) + 2 * mu_ * E
    J, Ci = np.linalg.det(A), np.linalg.inv(C)
    I1 = np.trace(C)
    I2 = 0.5 * (I1 ** 2 - np.trace(C @ C))
    return (2 * m["mu10"] * J ** (-2 / 3) * (np.eye(3) - I1 / 3 * Ci)
            + 2 * m["mu01"] * J ** (-4 / 3) * (I1 * np.eye(3) - C - 2 * I2 / 3 * Ci) + m["kappa"] * (J - 1) * J * Ci)


def cauchy_closed_form(A, m):
    """sigma = J^-1 A S(A) A^T, 6 doubles xx yy zz xy yz zx"""
    return snp.voigt(A @ second_pk(A, m) @ A.T / np.linalg.det(A))


def moduli(m):
    return sum(snp.lame(m)) if m["kind"] == "svk" else m["kappa"] + m["mu10"] + m["mu01"]


def perturbed(o, sigma=1e-3, vsigma=1e-1, seed=12345):
    """helpers.perturbed_state-style noise on all coefficients -> (x [n_coef, 3], v [3 n_coef])"""
    rng = np.random.default_rng(seed)
    X = coefficients(o)
    return X + rng.normal(0.0, sigma, X.shape), rng.normal(0.0, vsigma, X.shape).reshape(-1)


def set_state(o, x):
    o.x, o.y, o.z = (np.ascontiguousarray(x[:, c]) for c in range(3))


FD_EPS = 1e-4   # step of the energy-derivative check: truncation c eps^2 there is >= 100 x the rounding (tests/test_ancf_stress_np.py)


def energy_fd(energy, force, x, eps, seed=3):
    """(central difference of `energy` along a random direction dx at +-eps, force(x) . dx, dx)"""
    rng = np.random.default_rng(seed)
    dx = rng.normal(0.0, 1.0, x.shape)
    dx /= np.abs(dx).max()
    fd = (energy(x + eps * dx) - energy(x - eps * dx)) / (2 * eps)
    return fd, float(force(x) @ dx.reshape(-1)), dx
