"""The NumPy restatement tests/ancf_obstacles_np.py of the ANCF obstacle contact (DESIGN 3e'), pinned without a GPU so that
tests/test_gpu_ancf_obstacles.py compares the kernels with something already checked: the weights against the face
areas, the force against the derivative of the energy, the Hessian against the derivative of the force, symmetry and
positive semi-definiteness, and the new symbols and members."""
import numpy as np
import pytest

from tests import ancf_obstacles_np as aonp
from tests import ancf_stress_np as anp
from tests.helpers import tl

EPS = np.finfo(float).eps
H_STEP = 1e-2
PROBLEMS = {"beam2": lambda: anp.beam_line(2), "plate2x2": lambda: anp.shell_plate(2, 2)}
NEW = ("tlfea_ancf_set_obstacles", "tlfea_ancf_update_obstacle", "tlfea_ancf_clear_obstacles",
       "tlfea_ancf_get_obstacle_forces", "tlfea_ancf_get_obstacle_resultant", "tlfea_ancf_get_surface_points",
       "tlfea_ancf_retrieve_contact_points")
# Step of the central differences.  Away from the switching surfaces (d = 0, d(x_prev) = 0, |u| = eps_v h; the state
# below keeps every point > 100 FD_EPS from them, asserted) Phi is smooth.  Truncation: eps^2 / 6 x the third derivative
# along dx, relative to the first: 0 for a half-space's normal term (quadratic), <= (eps / R)^2 for a sphere, and for
# friction 2 / eps_f^2 on the stick branch (f0 is cubic in |u|), 1 / |u|^2 > on the sliding one; with eps_f = eps_v h
# = 5e-3 and |u| > eps_f that is (1e-6 / 5e-3)^2 = 4e-8.  Rounding: the energy difference carries 2 EPS |Phi| per term,
# Phi / (eps |grad Phi|) ~ depth / eps = 1e-2 / 1e-6, so 4e-12 per term x 64 terms.  FD_TOL = 1e-6 leaves a factor 25.
FD_EPS = 1e-6
FD_TOL = 1e-6
EPS_V = 0.5


def obstacles(pname, mu_plane, mu_sphere):
    """a half-space through the lower part of the mesh and a sphere dipping into it from above"""
    if pname == "beam2":
        return [dict(kind=0, p=np.array([0.0, 0.0, -0.04]), n=np.array([0.0, 0.0, 1.0]), kappa=3e7, mu=mu_plane,
                     eps_v=EPS_V, vel=np.array([0.2, 0.1, 0.0])),
                dict(kind=1, p=np.array([0.6, 1.0, 0.23]), radius=0.2, kappa=5e7, mu=mu_sphere, eps_v=EPS_V,
                     vel=np.array([0.0, -0.1, 0.05]))]
    return [dict(kind=0, p=np.array([0.0, 0.0, -0.03]), n=np.array([0.0, 0.0, 1.0]), kappa=3e7, mu=mu_plane, eps_v=EPS_V,
                 vel=np.array([0.2, 0.1, 0.0])),
            dict(kind=1, p=np.array([3.2, 1.6, 1.97]), radius=2.0, kappa=5e7, mu=mu_sphere, eps_v=EPS_V,
                 vel=np.array([0.0, -0.1, 0.05]))]


def state(prob, slide):
    """(x_prev, x): noise on the reference; `slide` moves x far enough for |u| > eps_v h (the sliding branch)"""
    rng = np.random.default_rng(7)
    X = aonp.reference(prob)
    xp = X + rng.normal(0, 2e-3, X.shape)
    x = xp + rng.normal(0, 1e-4, X.shape)
    if slide:
        x[0::4] += np.array([0.02, -0.015, 0.0])
    return xp, x


def clear_of_switches(prob, obs, x, xp, margin):
    r, r0 = aonp.positions(prob, x), aonp.positions(prob, xp)
    for o in obs:
        for q, q0 in zip(r.reshape(-1, 3), r0.reshape(-1, 3)):
            d, d0 = aonp.onp.distance(o, q)[0], aonp.onp.distance(o, q0)
            u = q - q0 - H_STEP * o["vel"]
            u = u - (d0[1] @ u) * d0[1]
            if min(abs(d), abs(d0[0]), abs(np.linalg.norm(u) - o["eps_v"] * H_STEP)) <= margin:
                return False
    return True


@pytest.mark.parametrize("pname", sorted(PROBLEMS))
def test_weights_sum_to_the_face_areas(pname):
    prob = PROBLEMS[pname]()
    L, W, H = prob[5]
    w = aonp.weights(prob)
    area = 2 * L * W if prob[0] == 3443 else 2 * L * W + 2 * L * H
    assert w.shape == (prob[4].shape[0], 32)
    assert np.abs(w.sum(axis=1) - area).max() <= 64 * EPS * area
    Sv = aonp.shape_values(prob[0], prob[5])
    assert np.abs(Sv[:, 0::4].sum(axis=1) - 1.0).max() <= 64 * EPS      # the position functions sum to one
    X = aonp.reference(prob)
    r = aonp.positions(prob, X)
    half = H / 2
    if prob[0] == 3443:                                                  # the reference points lie on the two faces
        assert np.abs(np.abs(r[:, :, 2]) - half).max() <= 64 * EPS
    else:
        assert np.abs(np.abs(r[:, :16, 1] - X[0, 1]) - W / 2).max() <= 64 * EPS and np.abs(np.abs(r[:, 16:, 2]) - half).max() <= 64 * EPS


@pytest.mark.parametrize("slide", [False, True])
@pytest.mark.parametrize("mus", [(0.4, 0.0), (0.0, 0.3)])
@pytest.mark.parametrize("pname", sorted(PROBLEMS))
def test_force_and_hessian_are_derivatives(pname, mus, slide):
    """f = -dPhi/dx along a random direction, and every column of the Hessian = -d f / d x_k, by central differences at
    FD_EPS.  A sphere's block is the Gauss-Newton one: the term it leaves out (`curvature`) is added before comparing."""
    prob = PROBLEMS[pname]()
    obs = obstacles(pname, *mus)
    xp, x = state(prob, slide)
    assert clear_of_switches(prob, obs, x, xp, 100 * FD_EPS)
    ref = aonp.assemble(prob, obs, x, xp, H_STEP)
    assert np.count_nonzero(ref["gap"] < 0) >= 8
    fric = [o for o in obs if o["mu"] > 0][0]
    r, r0 = aonp.positions(prob, x), aonp.positions(prob, xp)
    ys = [np.linalg.norm((q - q0 - H_STEP * fric["vel"]) - (n0 @ (q - q0 - H_STEP * fric["vel"])) * n0)
          for q, q0 in zip(r.reshape(-1, 3), r0.reshape(-1, 3))
          for d0, n0 in [aonp.onp.distance(fric, q0)] if d0 < 0]
    assert ys and (min(ys) > EPS_V * H_STEP if slide else max(ys) < EPS_V * H_STEP)     # the branch this case is about
    rng = np.random.default_rng(3)
    dx = rng.normal(0, 1, x.shape)
    dx /= np.abs(dx).max()
    fd = (aonp.energy(prob, obs, x + FD_EPS * dx, xp, H_STEP) - aonp.energy(prob, obs, x - FD_EPS * dx, xp, H_STEP)) / (2 * FD_EPS)
    fdx = float(np.sum(ref["force"] * dx))
    print(f"{pname} {mus} slide={slide}: -dPhi {-fd:.12e}  f.dx {fdx:.12e}")
    assert abs(fd + fdx) <= FD_TOL * np.abs(ref["force"]).sum()
    Hfull = (ref["hessian"] + ref["curvature"]) / H_STEP
    scale = np.abs(Hfull).max()
    worst = 0.0
    for k in range(x.size):
        e = np.zeros(x.size)
        e[k] = FD_EPS
        e = e.reshape(x.shape)
        col = -(aonp.assemble(prob, obs, x + e, xp, H_STEP)["force"] - aonp.assemble(prob, obs, x - e, xp, H_STEP)["force"]) / (2 * FD_EPS)
        worst = max(worst, np.abs(col.reshape(-1) - Hfull[:, k]).max())
    print(f"  worst column error {worst / scale:.3e} of the largest entry")
    assert worst <= FD_TOL * scale


@pytest.mark.parametrize("pname", sorted(PROBLEMS))
def test_hessian_is_symmetric_and_psd(pname):
    prob = PROBLEMS[pname]()
    for slide in (False, True):
        xp, x = state(prob, slide)
        Hd = aonp.assemble(prob, obstacles(pname, 0.4, 0.3), x, xp, H_STEP)["hessian"]
        assert np.abs(Hd).max() > 0
        assert np.abs(Hd - Hd.T).max() <= 16 * EPS * np.abs(Hd).max()
        ev = np.linalg.eigvalsh(0.5 * (Hd + Hd.T))
        assert ev.min() >= -1e-12 * ev.max()


def test_symbols_and_members():
    syms = tl.exported_symbols()
    assert all(s in syms for s in NEW)
    for cls in (tl.GPU_ANCF3243_Data, tl.GPU_ANCF3443_Data):
        for name in ("SetRigidObstacles", "UpdateRigidObstacle", "ClearRigidObstacles", "GetObstacleForces",
                     "GetObstacleResultant", "GetSurfacePointWeights", "RetrieveContactPointsToCPU"):
            assert name in vars(cls.__mro__[1]), name                    # the ANCF mirror's own, not the T10 ones
