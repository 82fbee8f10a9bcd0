"""The NumPy restatement tests/t10_loads_np.py of the surface loads on T10 boundary faces (DESIGN 3h'), pinned without a GPU
so that tests/test_gpu_t10_loads.py compares the kernel with something already checked: the boundary faces of boxes and of a
closed curved surface, the traction's closed form, the degree of the pressure rule, the closed-surface resultant and moment,
the pressure as the derivative of the enclosed volume, and the hydrostatic state against the oracle's internal force; and the
new symbols, members, struct, refusals and driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import orc
from tests import obstacles_np as onp
from tests import t10_loads_np as lnp
from tests.helpers import MATERIALS, MESHES, load_mesh, make_oracle, tl

mu = tl.mesh_utils
EPS = np.finfo(float).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
NEW = ("tlfea_t10_get_boundary_faces", "tlfea_t10_set_surface_loads", "tlfea_t10_update_load_scale")
T_VEC = np.array([120.0, -80.0, 300.0])
LAM = 0.98


def sphere():
    _, X = mu.FEAT10_read_nodes(os.path.join(MESHES, "sphere.1.node"))
    _, conn = mu.FEAT10_read_elements(os.path.join(MESHES, "sphere.1.ele"))
    return X, conn


def bent(X):
    """a smooth displacement that is not affine, a twentieth of the mesh size"""
    return X + 0.05 * np.abs(X).max() * np.sin(3.0 * X[:, [1, 2, 0]] / np.abs(X).max())


def hydrostatic_pressure(m, lam=LAM):
    """x = lam X under SVK: S = (3 lam_L + 2 mu) (lam^2 - 1) / 2 I, Cauchy stress S / lam, so p = -S / lam holds it"""
    lam_l = m["E"] * m["nu"] / ((1 + m["nu"]) * (1 - 2 * m["nu"]))
    g = m["E"] / (2 * (1 + m["nu"]))
    return -(3 * lam_l + 2 * g) * (lam ** 2 - 1) / (2 * lam)


# ---- boundary faces -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [(1, 1, 1), (2, 3, 1)])
def test_boundary_faces_of_a_box(cells):
    nx, ny, nz = cells
    dims = (1.5, 1.0, 0.8)
    X, conn = mu.structured_t10_box(nx, ny, nz, *dims)
    elem, lf, nodes = lnp.boundary_faces(X, conn)
    assert len(elem) == 2 * 2 * (nx * ny + ny * nz + nx * nz)
    cen, nrm, area = lnp.face_geometry(X, nodes)
    surface = 2 * (dims[0] * dims[1] + dims[1] * dims[2] + dims[0] * dims[2])
    assert abs(area.sum() - surface) <= 64 * EPS * surface
    assert np.all(np.einsum("ij,ij->i", nrm, cen - 0.5 * np.array(dims)) > 0)          # away from the centre of the box
    assert np.all(np.abs(np.abs(nrm).max(axis=1) - 1.0) <= 8 * EPS)                     # and along an axis
    order = elem.astype(np.int64) * 4 + lf
    assert np.all(np.diff(order) > 0)                                                   # ascending (element, local face)
    for k in range(len(elem)):                                                          # the element's own nodes
        assert sorted(nodes[k]) == sorted(conn[elem[k]][list(onp.FACES[lf[k]])])
        for m, (a, b) in enumerate(((0, 1), (1, 2), (0, 2))):                           # mid-edge nodes follow their corners
            assert np.abs(X[nodes[k, 3 + m]] - 0.5 * (X[nodes[k, a]] + X[nodes[k, b]])).max() <= 8 * EPS


def test_boundary_faces_of_the_sphere_close_the_surface():
    X, conn = sphere()
    elem, lf, nodes = lnp.boundary_faces(X, conn)
    edges = {}
    for nd in nodes:
        for a, b in ((0, 1), (1, 2), (2, 0)):
            edges.setdefault((min(nd[a], nd[b]), max(nd[a], nd[b])), []).append((nd[a], nd[b]))
    assert all(len(v) == 2 for v in edges.values())
    assert all(v[0] == v[1][::-1] for v in edges.values())          # and the two faces run along it in opposite directions
    _, nrm, area = lnp.face_geometry(X, nodes)
    total = onp.surface_weights(X, conn).sum()
    assert abs(area.sum() - total) <= 64 * EPS * total
    assert np.all(np.diff(elem.astype(np.int64) * 4 + lf) > 0)


# ---- traction -----------------------------------------------------------------------------------------------------------------
def test_traction_on_straight_faces():
    X, conn = mu.structured_t10_box(2, 3, 1, 1.5, 1.0, 0.8)
    _, _, nodes = lnp.boundary_faces(X, conn)
    _, _, area = lnp.face_geometry(X, nodes)
    for k in (0, 7, len(nodes) - 1):
        rows = lnp.traction_rows(X, nodes[k], T_VEC)
        bound = 8 * EPS * area[k] * np.abs(T_VEC).max()
        assert np.abs(rows[:3]).max() <= bound                                          # corners: 0
        assert np.abs(rows[3:] - area[k] * T_VEC / 3.0).max() <= bound                  # mid-edge nodes: t A / 3
    faces = np.arange(len(nodes))
    f = lnp.traction_force(X, nodes, faces, T_VEC)
    assert np.abs(f.sum(axis=0) - area.sum() * T_VEC).max() <= 64 * EPS * area.sum() * np.abs(T_VEC).max()


# ---- pressure -----------------------------------------------------------------------------------------------------------------
def test_pressure_rule_has_degree_four():
    """N_a (r_xi x r_eta) has degree 2 + 1 + 1 = 4: the 6-point rule equals a rule of degree 10 (6 x 6 collapsed Gauss
    points) to rounding on a face whose mid-edge nodes are displaced; the 3-point rule of degree 2 does not."""
    X, conn = mu.structured_t10_box(1, 1, 1)
    _, _, nodes = lnp.boundary_faces(X, conn)
    rng = np.random.default_rng(5)
    x = X.copy()
    mids = np.unique(nodes[:, 3:])
    x[mids] += rng.normal(0, 0.08, (len(mids), 3))
    worst, worst3 = 0.0, np.inf
    for nd in nodes:
        fine = lnp.pressure_rows(x, nd, 3e4, lnp.rule_duffy(6))
        scale = np.abs(fine).max()
        worst = max(worst, np.abs(lnp.pressure_rows(x, nd, 3e4) - fine).max() / scale)
        worst3 = min(worst3, np.abs(lnp.pressure_rows(x, nd, 3e4, lnp.rule3()) - fine).max() / scale)
    print(f"6-point rule {worst:.2e}  3-point rule {worst3:.2e}")
    assert worst <= 1e-15
    assert worst3 > 1e-6


@pytest.mark.parametrize("mesh", ["sphere", "box"])
def test_pressure_on_a_closed_surface_has_no_resultant_and_no_moment(mesh):
    """The integral of n dA and of r x n dA over a closed surface vanish, and the rule is exact: what is left is rounding,
    within 64 EPS x the sum of the absolute terms (the bound of test_ancf_loads_np.test_mesh_independence)."""
    X, conn = sphere() if mesh == "sphere" else mu.structured_t10_box(2, 3, 1, 1.5, 1.0, 0.8)
    _, _, nodes = lnp.boundary_faces(X, conn)
    x = bent(X)
    res, mom, res_abs, mom_abs = np.zeros(3), np.zeros(3), 0.0, 0.0
    for nd in nodes:
        rows = lnp.pressure_rows(x, nd, 2.5e4)
        res += rows.sum(axis=0)
        mom += np.cross(x[nd], rows).sum(axis=0)
        res_abs += np.abs(rows).sum()
        mom_abs += 2.0 * (np.abs(x[nd]).max(axis=1)[:, None] * np.abs(rows)).sum()
    print(mesh, np.abs(res).max() / (EPS * res_abs), np.abs(mom).max() / (EPS * mom_abs), "EPS of the absolute sums")
    assert res_abs > 0
    assert np.abs(res).max() <= 64 * EPS * res_abs
    assert np.abs(mom).max() <= 64 * EPS * mom_abs


@pytest.mark.parametrize("mesh", ["sphere", "box"])
def test_pressure_is_the_derivative_of_the_volume(mesh):
    """f = -p dV/dx with V the sum of the current element volumes (det J is cubic: the 5-point rule is exact).  One
    coordinate of one node enters one row of every J only, so V is LINEAR in it and the central difference is exact but
    for the rounding of V: two values, each a sum of 5 E products rounded within 32 EPS V, over 2 step."""
    X, conn = sphere() if mesh == "sphere" else mu.structured_t10_box(2, 3, 1, 1.5, 1.0, 0.8)
    _, _, nodes = lnp.boundary_faces(X, conn)
    rule = orc.keast5()
    x = bent(X)
    p = 2.5e4
    f = lnp.pressure_force(x, nodes, range(len(nodes)), p)
    V = lnp.volume(x, conn, rule)
    step = 1e-2 * np.abs(X).max()
    inner = np.setdiff1d(np.arange(X.shape[0]), nodes)
    picks = [nodes[0, 0], nodes[3, 4], nodes[len(nodes) // 2, 1], nodes[-1, 5]] + ([inner[0]] if len(inner) else [])
    assert np.abs(f[nodes[0, 0]]).max() > 0
    for i in picks:
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += step
            xm[i, c] -= step
            fd = -p * (lnp.volume(xp, conn, rule) - lnp.volume(xm, conn, rule)) / (2 * step)
            assert abs(f[i, c] - fd) <= p * 64 * EPS * V / (2 * step)
    if len(inner):
        assert not f[inner].any()


@pytest.mark.parametrize("mesh", ["beam_3x2x1", "sphere"])
def test_hydrostatic_state_without_a_solver(mesh):
    """x = lam X, SVK, the pressure that holds it on every boundary face: the oracle's internal force equals the load on
    the boundary rows and vanishes inside.  Measured here: 3.5e-14 (beam_3x2x1) and 6.8e-14 (sphere.1) of the largest
    internal-force row, against the bound 1e-12."""
    X, conn = sphere() if mesh == "sphere" else load_mesh(mesh)
    m = MATERIALS["svk"]
    o = make_oracle(X, conn, m)
    o.x[:], o.y[:], o.z[:] = LAM * X[:, 0], LAM * X[:, 1], LAM * X[:, 2]
    fint = o.internal_force().reshape(-1, 3)
    _, _, nodes = lnp.boundary_faces(X, conn)
    load = lnp.pressure_force(LAM * X, nodes, range(len(nodes)), hydrostatic_pressure(m))
    scale = np.abs(fint).max()
    inner = np.setdiff1d(np.arange(X.shape[0]), nodes)
    err = np.abs(fint - load).max() / scale
    print(mesh, f"boundary and interior rows {err:.2e} of the largest internal-force row {scale:.3e}")
    assert scale > 0 and err <= 1e-12
    if len(inner):
        assert not load[inner].any() and np.abs(fint[inner]).max() <= 1e-12 * scale


# ---- surface of the feature ---------------------------------------------------------------------------------------------------
def test_symbols_members_and_struct_layout():
    syms = tl.exported_symbols()
    assert all(s in syms for s in NEW)
    for name in ("GetBoundaryFaces", "AddFaceTraction", "AddFacePressure", "SetFaceLoadScale", "ClearLoads", "GetLoadForces",
                 "GetLoadResultant"):
        assert name in vars(tl.GPU_FEAT10_Data), name
    txt = open(tl.binding.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\} tlfea_t10_surface_load;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert decl == ["int kind", "double value[3]", "double scale", "const int *faces", "int n_faces"]
    S = tl.binding.T10SurfaceLoadC
    assert [f[0] for f in S._fields_] == ["kind", "value", "scale", "faces", "n_faces"]
    assert (S.kind.offset, S.value.offset, S.scale.offset, S.faces.offset, S.n_faces.offset) == (0, 8, 32, 40, 48)
    assert C.sizeof(S) == 56
    # declared after the existing loads block
    assert txt.index("tlfea_get_load_resultant(") < txt.index("tlfea_t10_get_boundary_faces(")
    facade = open(os.path.join(HOST, "tlfea_facade.h")).read()
    for name in ("GetBoundaryFaces", "AddFaceTraction", "AddFacePressure", "SetFaceLoadScale"):
        assert name in facade, name


def test_refusals_without_a_gpu():
    """what the mirror refuses before it reaches the C-ABI (which refuses the same again: tests/test_gpu_t10_loads.py)"""
    d = tl.GPU_FEAT10_Data(6, 27)                                        # not initialised: nothing below touches the GPU
    d._n_boundary_faces = 12
    with pytest.raises(ValueError, match="outside 0..11"):
        d.AddFacePressure([12], 1e4)
    with pytest.raises(ValueError, match="negative"):
        d.AddFaceTraction([-1], T_VEC)
    with pytest.raises(ValueError, match="twice"):
        d.AddFacePressure([0, 1, 0], 1e4)
    with pytest.raises(ValueError, match="non-empty"):
        d.AddFacePressure([], 1e4)
    with pytest.raises(ValueError, match="integers"):
        d.AddFacePressure([0.5], 1e4)
    with pytest.raises(ValueError, match="finite"):
        d.AddFacePressure([0], float("nan"))
    with pytest.raises(ValueError, match="finite"):
        d.AddFacePressure([0], 1e4, scale=float("inf"))
    with pytest.raises(ValueError, match="3-vector"):
        d.AddFaceTraction([0], [1.0, 2.0])
    with pytest.raises(ValueError, match="3-vector"):
        d.AddFaceTraction([0], [1.0, 2.0, float("nan")])
    with pytest.raises(ValueError, match="kind must be"):
        tl.loads.FaceLoad(2, [0], 1.0)
    d._face_loads = [tl.loads.FaceLoad(1, [0], 1.0)] * 16
    with pytest.raises(ValueError, match="at most 16"):
        d.AddFacePressure([0], 1e4)
    with pytest.raises(ValueError, match="outside the 16"):
        d.SetFaceLoadScale(16, 1.0)
    with pytest.raises(ValueError, match="finite"):
        d.SetFaceLoadScale(0, float("nan"))
    shell = tl.GPU_ANCF3443_Data(9, 4)
    for call in (lambda: shell.GetBoundaryFaces(), lambda: shell.AddFacePressure([0], 1e4),
                 lambda: shell.AddFaceTraction([0], T_VEC), lambda: shell.SetFaceLoadScale(0, 1.0)):
        with pytest.raises(ValueError, match="T10 objects only"):
            call()


def test_pressurized_block_driver_builds(tmp_path):
    lib_dir = os.path.join(ROOT, "total-lagrangian-fea_amd")
    out = tmp_path / "test_pressurized_block"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(out),
                           os.path.join(HOST, "test_pressurized_block.cc"), "-L" + lib_dir, "-ltlfea_hip",
                           "-Wl,-rpath," + lib_dir])
    assert out.exists()
