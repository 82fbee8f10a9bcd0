"""Hydroelastic contact on the GPU (csrc/contact_kernels.hip through the tlfea_contact_* C-ABI): broadphase against a
brute-force box test, patches and forces against the NumPy restatement (tests/contact_np.py), closed-form forces
between two stacked boxes, bitwise determinism, and a coupled contact + implicit Newton run against the CPU oracle."""
import importlib
import os

import numpy as np
import pytest

from oracle import orc
from tests import contact_np as cnp
from tests.helpers import MESHES, make_gpu, make_oracle, tl

pytestmark = pytest.mark.gpu

SPHERE = os.path.join(MESHES, "sphere.1")
NPZ = os.path.join(MESHES, "sphere.1.uncompressed.npz")
R = 0.15


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if tl.device_count() < 1:
        pytest.fail("GPU tests need a visible GPU")
    return t


def two_spheres(offset):
    mm = tl.MeshManager()
    for _ in range(2):
        assert mm.LoadMesh(SPHERE + ".node", SPHERE + ".ele") >= 0
        assert mm.LoadScalarFieldFromNpz(mm.GetNumMeshes() - 1, NPZ)
    mm.TranslateMesh(1, *offset)
    return mm, mm.GetAllNodes().copy(), mm.GetAllElements().copy(), mm.GetAllScalarFields(), mm.GetAllElementMeshIds()


def dev_nodes(torch, X):
    return torch.as_tensor(np.ascontiguousarray(X.T).reshape(-1), device="cuda")


def disp_err_ok(xg, xo, X):
    """The parity bar of the Newton tests: 1e-10 of the largest displacement plus 8 ulp of the coordinates."""
    floor = 8 * np.finfo(np.float64).eps * np.max(np.abs(xo))
    return np.max(np.abs(xg - xo)) <= 1e-10 * np.max(np.abs(xo - X)) + floor


def rel_close(a, b, tol, scale=None):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    s = scale if scale is not None else max(np.max(np.abs(b)), 1e-300)
    return np.max(np.abs(a - b)) <= tol * s if a.size else True


@pytest.mark.parametrize("self_collision", [False, True])
def test_broadphase_is_exact_and_ordered(torch, self_collision):
    rng = np.random.default_rng(7)
    mm, X, conn, p, mesh = two_spheres((rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.25))
    c = tl.HydroelasticPatchCollisionSystem(mm, X, conn, p, mesh, self_collision)
    xd = dev_nodes(torch, X)
    c.BindNodesDevicePtr(xd.data_ptr(), X.shape[0])
    c.Step()
    pairs, _ = c.RetrieveResults()
    ref = cnp.brute_force_pairs(X, conn, mesh, self_collision)
    assert len(ref) > 0
    assert np.array_equal(pairs, ref)  # same set, and the canonical (i, j) order
    if self_collision:
        assert np.any(mesh[pairs[:, 0]] == mesh[pairs[:, 1]])
    c.Step()
    again, _ = c.RetrieveResults()
    assert np.array_equal(again, pairs)
    c.Destroy()


def test_patches_match_numpy(torch):
    mm, X, conn, p, mesh = two_spheres((0.02, -0.01, 0.26))
    c = tl.HydroelasticPatchCollisionSystem(mm, X, conn, p, mesh, False)
    xd = dev_nodes(torch, X)
    c.BindNodesDevicePtr(xd.data_ptr(), X.shape[0])
    c.Step()
    pairs, patches = c.RetrieveResults()
    ref, fref = cnp.contact(X, conn, p, mesh, pairs)
    assert c.GetNumPatches() == sum(r["isValid"] for r in ref) > 0
    for g, r in zip(patches, ref):
        assert (g.tetA_idx, g.tetB_idx) == (r["tetA"], r["tetB"])
        assert (g.isValid, g.validOrientation) == (r["isValid"], r["validOrientation"])
        if not r["isValid"]:
            continue
        # (the vertex count may differ: a clip plane through a polygon vertex adds a duplicate on one side of rounding)
        assert abs(g.area - r["area"]) <= 1e-12 * r["area"]
        assert rel_close(g.centroid, r["centroid"], 1e-12, R)
        assert rel_close(g.normal, r["normal"], 1e-12, 1.0)
        for k in ("g_A", "g_B"):
            assert abs(getattr(g, k) - r[k]) <= 1e-12 * abs(r[k])
        assert abs(g.p_equilibrium - r["p_equilibrium"]) <= 1e-12 * np.max(np.abs(p))
    assert rel_close(c.RetrieveForces(), fref, 1e-12)
    c.Destroy()


# ---- two stacked boxes: closed-form answers -------------------------------------------------------------------------
W, KA, KB, DELTA = 1.0, 1.0e5, 2.0e5, 0.3
ZSTAR = 1.0 - KB * DELTA / (KA + KB)       # 0.8: between the node planes 0.75 / 1.0 (A) and 0.7 / 0.95 (B)
PEQ = KA * KB * DELTA / (KA + KB)


def boxes(swap_ids=False):
    Xa, ca = tl.mesh_utils.structured_t10_box(4, 4, 2, W, W, 1.0)
    Xb, cb = Xa.copy(), ca.copy()
    z0 = 1.0 - DELTA
    Xb[:, 2] += z0
    X = np.concatenate([Xa, Xb])
    conn = np.concatenate([ca, cb + Xa.shape[0]]).astype(np.int32)
    p = np.concatenate([KA * (1.0 - Xa[:, 2]), KB * (Xb[:, 2] - z0)])
    mesh = np.concatenate([np.zeros(len(ca)), np.ones(len(cb))]).astype(np.int32)
    if swap_ids:
        mesh = 1 - mesh
    return X, conn, p, mesh, Xa.shape[0]


def box_forces(torch, vel_b=None, damping=0.0, friction=0.0, swap_ids=False):
    X, conn, p, mesh, na = boxes(swap_ids)
    c = tl.HydroelasticPatchCollisionSystem(None, X, conn, p, mesh, False)
    xd = dev_nodes(torch, X)
    c.BindNodesDevicePtr(xd.data_ptr(), X.shape[0])
    vd = None
    if vel_b is not None:
        v = np.zeros((X.shape[0], 3))
        v[na:] = vel_b
        vd = torch.as_tensor(v.reshape(-1), device="cuda")
    c.Step(tl.CollisionSystemInput(d_vel_xyz=vd.data_ptr() if vd is not None else 0),
           tl.CollisionSystemParams(damping, friction))
    _, patches = c.RetrieveResults()
    f = c.RetrieveForces().reshape(-1, 3)
    c.Destroy()
    return X, f, patches, na


def test_stacked_boxes_closed_form(torch):
    X, f, patches, na = box_forces(torch)
    valid = [q for q in patches if q.isValid and q.validOrientation]
    assert abs(sum(q.area for q in valid) - W * W) <= 1e-12 * W * W
    for q in valid:
        assert abs(q.centroid[2] - ZSTAR) <= 1e-12 and np.allclose(q.normal, [0, 0, 1], rtol=0, atol=1e-14)
    FB, FA = f[na:].sum(axis=0), f[:na].sum(axis=0)
    expect = np.array([0.0, 0.0, PEQ * W * W])
    assert np.max(np.abs(FB - expect)) <= 1e-12 * expect[2]
    assert np.max(np.abs(FA + expect)) <= 1e-12 * expect[2]
    assert np.max(np.abs(f.sum(axis=0))) <= 1e-12 * expect[2]
    ctr = np.array([W / 2, W / 2, ZSTAR])
    moment = np.cross(X - ctr, f).sum(axis=0)
    assert np.max(np.abs(moment)) <= 1e-12 * expect[2] * W


def test_stacked_boxes_damping_friction_and_ids(torch):
    _, f0, _, na = box_forces(torch)
    N0 = f0[na:, 2].sum()
    d, v = 0.2, 0.5
    _, f, _, _ = box_forces(torch, vel_b=[0, 0, -v], damping=d)
    assert abs(f[na:, 2].sum() - N0 * (1 + d * v)) <= 1e-12 * N0
    _, f, _, _ = box_forces(torch, vel_b=[0, 0, 2.0 / d], damping=d)
    assert np.max(np.abs(f)) == 0.0
    mu, u = 0.8, 0.01
    _, f, _, _ = box_forces(torch, vel_b=[u, 0, 0], friction=mu)
    FB = f[na:].sum(axis=0)
    assert abs(FB[0] + mu * N0 * u / (u + 1e-3)) <= 1e-12 * N0 and abs(FB[1]) <= 1e-12 * N0
    assert abs(FB[2] - N0) <= 1e-12 * N0
    _, fs, _, _ = box_forces(torch, swap_ids=True)
    assert np.max(np.abs(fs - f0)) <= 1e-12 * np.max(np.abs(f0))


def test_contact_step_is_bitwise_deterministic(torch):
    mm, X, conn, p, mesh = two_spheres((0.01, 0.02, 0.27))
    xd = dev_nodes(torch, X)
    v = torch.as_tensor(np.random.default_rng(3).normal(0, 0.3, X.size), device="cuda")
    out = []
    for _ in range(2):
        c = tl.HydroelasticPatchCollisionSystem(mm, X, conn, p, mesh, False)
        c.BindNodesDevicePtr(xd.data_ptr(), X.shape[0])
        for _ in range(2):
            c.Step(tl.CollisionSystemInput(d_vel_xyz=v.data_ptr()), tl.CollisionSystemParams(0.2, 0.8))
            out.append(c.RetrieveForces())
        c.Destroy()
    assert np.max(np.abs(out[0])) > 0
    for o in out[1:]:
        assert o.tobytes() == out[0].tobytes()


def test_coupled_sphere_drop_matches_oracle(torch):
    """Top sphere 2 mm above the pinned bottom one (node to node), moving down at 0.5 m/s: 30 steps of contact -> f_ext -> implicit
    Newton on the GPU, against the oracle fed with the NumPy contact force of its own state."""
    gap, v0, dt = 2e-3, 0.5, 5e-4
    _, X1, _, _, _ = two_spheres((0.0, 0.0, 0.0))
    n1 = X1.shape[0] // 2   # the faceted sphere: its lowest node 2 mm above the other copy's highest node
    mm, X, conn, p, mesh = two_spheres((0.0, 0.0, X1[:n1, 2].max() - X1[:n1, 2].min() + gap))
    N = X.shape[0]
    n0 = mm.GetMeshInstance(0).num_nodes
    fixed = np.where(X[:n0, 2] < X[:n0, 2].mean())[0].astype(np.int32)
    mat = dict(kind="svk", E=4e6, nu=0.3, rho0=3500.0, eta=1e4, lamd=1e4)
    base = np.zeros(3 * N)
    mass = 3500.0 * 4.0 / 3.0 * np.pi * R ** 3
    base[3 * np.arange(n0, N) + 2] = -9.81 * mass / (N - n0)
    o, d = make_oracle(X, conn, mat, fixed, base.copy()), make_gpu(X, conn, mat, fixed, base)  # the oracle keeps its array
    prm = (1e-8, 0.0, 1e-10, 1e12, 3, 5, dt)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(*prm))
    s.SetLinSolveOpts(tl.LinSolveOpts(1e-13, 20000, 10))
    vel = np.zeros(3 * N)
    vel[3 * np.arange(n0, N) + 2] = -v0
    s.SetVelocity(vel, vel)
    o.v[:] = vel
    o.v_prev[:] = vel
    c = tl.HydroelasticPatchCollisionSystem(mm, X, conn, p, mesh, False)
    c.BindElementData(d)
    c.SetBaseForce(base)
    par = importlib.import_module("total-lagrangian-fea_amd.partition")
    v_dev = torch.as_tensor(par._DevicePtr(s.GetVelocityGuessDevicePtr(), 3 * N), device="cuda")
    damping, friction = 0.2, 0.8
    max_patches, max_fz = 0, 0.0
    for step in range(30):
        c.Step(tl.CollisionSystemInput(d_vel_xyz=s.GetVelocityGuessDevicePtr()), tl.CollisionSystemParams(damping, friction))
        c.ApplyToElementData()
        xg = np.stack(d.RetrievePositionToCPU(), axis=1)
        vg = v_dev.cpu().numpy()
        fg = c.RetrieveForces()
        _, fn = cnp.contact(xg, conn, p, mesh, cnp.brute_force_pairs(xg, conn, mesh, False), vg, damping, friction)
        assert rel_close(fg, fn, 1e-12, max(np.max(np.abs(fn)), 1.0))
        assert np.array_equal(d.RetrieveExternalForceToCPU(), base + fg)
        max_patches = max(max_patches, c.GetNumPatches())
        max_fz = max(max_fz, fg.reshape(-1, 3)[n0:, 2].sum())
        xo = np.stack([o.x, o.y, o.z], axis=1)
        _, fo = cnp.contact(xo, conn, p, mesh, cnp.brute_force_pairs(xo, conn, mesh, False), o.v, damping, friction)
        o.f_ext[:] = base + fo
        s.Solve()
        o.newton_step(orc.NewtonParams(*prm), solver=0)
        xg = np.stack(d.RetrievePositionToCPU(), axis=1)
        assert disp_err_ok(xg, np.stack([o.x, o.y, o.z], axis=1), X), f"step {step}"
    assert max_patches > 0 and max_fz > 0
    c.Destroy()
    del s
    d.Destroy()


def test_sphere_drop_driver_matches_python_mirror(torch, tmp_path):
    """host/test_sphere_drop_collision (C++ facade: Step -> ApplyToElementData -> Solve) for 200 steps with the spheres
    touching nominally (--gap=0, 17.6 mm between the faceted surfaces): CSV schema, the top sphere's centre stays above
    0.30 - 0.03, the contact force on it exceeds its weight, and the CSV equals the same loop through the Python mirror."""
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "total-lagrangian-fea_amd", "host")
    subprocess.check_call(["make", "-C", host, "test_sphere_drop_collision"], stdout=subprocess.DEVNULL)
    steps, damping, friction = 200, 0.2, 0.8
    csv = tmp_path / "drop.csv"
    r = subprocess.run([os.path.join(host, "test_sphere_drop_collision"), str(damping), str(friction), "0", str(steps),
                        "0", f"--mesh_dir={MESHES}", f"--csv_path={csv}", "--gap=0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = csv.read_text().splitlines()
    assert lines[0] == "step,top_center_z,num_pairs,num_patches,contact_fz_top" and len(lines) == steps + 1
    got = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert np.array_equal(got[:, 0], np.arange(steps))
    weight = 3500.0 * 4.0 / 3.0 * np.pi * R * R * R * 9.81
    assert got[:, 1].min() > 0.30 - 0.03
    assert got[:, 3].max() > 0 and got[:, 4].max() > weight

    # the same loop through the Python mirror
    mm, X, conn, p, mesh = two_spheres((0.0, 0.0, 2.0 * R + 0.0))
    N = X.shape[0]
    ib, it = mm.GetMeshInstance(0), mm.GetMeshInstance(1)
    zb = X[:ib.num_nodes, 2]
    fixed = np.where(zb < zb.sum() / ib.num_nodes)[0].astype(np.int32)
    base = np.zeros(3 * N)
    base[3 * np.arange(it.node_offset, N) + 2] = 3500.0 * 4.0 / 3.0 * np.pi * R * R * R / it.num_nodes * -9.81
    d = make_gpu(X, conn, dict(kind="svk", E=4e6, nu=0.3, rho0=3500.0, eta=1e4, lamd=1e4), fixed, base)
    s = tl.SyncedNewtonSolver(d, d.get_n_constraint())
    s.Setup()
    s.SetParameters(tl.SyncedNewtonParams(1e-8, 0.0, 1e-10, 1e12, 3, 5, 5e-4))
    c = tl.HydroelasticPatchCollisionSystem(mm, X, conn, p, mesh, False)
    c.BindElementData(d)
    c.SetBaseForce(base)
    inp = tl.CollisionSystemInput(d_vel_xyz=s.GetVelocityGuessDevicePtr(), dt=5e-4)
    rows = []
    for step in range(steps):
        c.Step(inp, tl.CollisionSystemParams(damping, friction))
        c.ApplyToElementData()
        npair, npatch = c.GetNumContacts(), c.GetNumPatches()
        fz = c.RetrieveForces().reshape(-1, 3)[it.node_offset:, 2].sum()
        s.Solve()
        rows.append((step, d.RetrievePositionToCPU()[2][it.node_offset:].mean(), npair, npatch, fz))
    ref = np.array(rows)
    assert np.array_equal(got[:, 2:4], ref[:, 2:4])
    assert np.max(np.abs(got[:, 1] - ref[:, 1])) <= 1e-12 * np.max(np.abs(ref[:, 1]))
    assert np.max(np.abs(got[:, 4] - ref[:, 4])) <= 1e-12 * max(np.max(np.abs(ref[:, 4])), weight)
    c.Destroy()
    del s
    d.Destroy()
