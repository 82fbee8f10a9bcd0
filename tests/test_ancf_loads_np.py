"""The NumPy restatement tests/ancf_loads_np.py of the distributed loads of the ANCF kinds, pinned without a
GPU so that tests/test_gpu_ancf_loads.py compares the kernels with something already checked: gravity against the oracle's
mass matrix, traction against the face areas and the derivative of its work, pressure against a finer rule, the closed
form on a flat face, rigid motions and a refined mesh; and the new symbols, members, struct, refusals and driver."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ancf_loads_np as lnp
from tests import ancf_obstacles_np as aonp
from tests import ancf_stress_np as anp
from tests.helpers import MATERIALS, tl
from tests.test_linear_constraints import TIRE

mu = tl.mesh_utils
EPS = np.finfo(float).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
# the five shapes of tests/test_gpu_ancf_stress.SHAPES that the GPU tests use (that module needs no GPU to build them, but
# it is marked gpu as a whole, so the constructors are restated here)
SHAPES = {"beam1": lambda: anp.beam_line(1), "beam5": lambda: anp.beam_line(5), "shell1": lambda: anp.shell_plate(1, 1),
          "plate2x2": lambda: anp.shell_plate(2, 2), "strip3x1": lambda: anp.shell_plate(3, 1)}
NEW = ("tlfea_set_body_acceleration", "tlfea_ancf_set_surface_loads", "tlfea_ancf_update_load_scale", "tlfea_clear_loads",
       "tlfea_get_load_forces", "tlfea_get_load_resultant")
RHO = 1000.0
A_G = np.array([0.3, -0.2, -9.81])
T_VEC = np.array([120.0, -80.0, 300.0])
Q_ROT = anp.Q_ROT


def perturbed(prob, sigma=2e-3, seed=11):
    """noise on every coefficient of the reference, as scene() of the obstacle tests"""
    X = aonp.reference(prob)
    return X + np.random.default_rng(seed).normal(0, sigma, X.shape)


def face_area(prob, face):
    L, W, H = prob[5]
    return L * W if prob[0] == 3443 or face >= 2 else L * H


def all_elems(prob):
    return list(range(prob[4].shape[0]))


# ---- gravity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gravity_is_the_oracle_mass_times_the_acceleration_field(shape):
    """Two independent integrations of the same polynomial mass (the oracle's C code, NumPy here): the bound is rounding,
    1e-12 of the largest entry (sums of up to 147 products that went through the inverse of B)."""
    prob = SHAPES[shape]()
    m = dict(MATERIALS["svk"], rho0=RHO)
    M = anp.make_oracle(prob, m).mass_dense()
    assert np.abs(lnp.mass_matrix(prob, RHO) - M).max() <= 1e-12 * np.abs(M).max()
    f = lnp.gravity_force(prob, RHO, A_G)
    ref = M @ lnp.acceleration_field(M.shape[0], A_G)
    assert np.abs(f - ref).max() <= 1e-12 * np.abs(ref).max()
    L, W, H = prob[5]
    mass = RHO * prob[4].shape[0] * L * W * H
    assert np.abs(f[0::4].sum(axis=0) - mass * A_G).max() <= 1e-12 * mass * np.abs(A_G).max()


# ---- traction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_traction_resultant_and_work_derivative(shape):
    prob = SHAPES[shape]()
    x = perturbed(prob)
    rng = np.random.default_rng(3)
    for face in range(lnp.FACES[prob[0]]):
        el = all_elems(prob)
        f = lnp.traction_force(prob, face, el, T_VEC)
        area = face_area(prob, face) * len(el)
        assert np.abs(f[0::4].sum(axis=0) - area * T_VEC).max() <= 1e-12 * area * np.abs(T_VEC).max()
        # W = int t . r dA is linear in x: the central difference is exact up to the rounding of W, 2 EPS |W| / (2 step)
        dx = rng.normal(0, 1, x.shape)
        step = 1e-2
        fd = (lnp.traction_work(prob, x + step * dx, face, el, T_VEC) - lnp.traction_work(prob, x - step * dx, face, el, T_VEC)) / (2 * step)
        Wabs = abs(lnp.traction_work(prob, x, face, el, T_VEC)) + np.abs(f).sum()
        assert abs(fd - np.sum(f * dx)) <= 64 * EPS * Wabs / step


def test_traction_on_the_curved_tire_sums_to_the_point_weights():
    m = mu.ReadANCF3443MeshFromFile(TIRE)
    for e in range(0, m.n_elements, max(1, m.n_elements // 6)):
        prob = (3443, m.x12, m.y12, m.z12, np.asarray(m.element_connectivity)[e:e + 1],
                (float(m.element_L[e]), float(m.element_W[e]), float(m.element_H[e])))
        w = aonp.weights(prob)
        for face in (0, 1):
            f = lnp.traction_force(prob, face, [0], T_VEC)
            area = w[0, lnp.face_slice(3443, face)].sum()
            assert area > 0
            assert np.abs(f[0::4].sum(axis=0) - area * T_VEC).max() <= 1e-12 * area * np.abs(T_VEC).max()


# ---- pressure ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pressure_rule_is_exact_and_the_four_point_rule_is_not(shape):
    """Shell: S_a (r_xi x r_eta) has degree 3 + 2 + 3 = 8 in xi and in eta, so 5 x 5 Gauss (degree 9) equals 8 x 8 to
    rounding and 4 x 4 (degree 7) does not.  Beam: degree 3 + 2 + 1 = 6 along xi and 2 across, so the 4-point rule would
    also be exact there; the kernels still use 5 x 2 (one table layout per kind), and the 3-point rule (degree 5) is the
    one that fails."""
    prob = SHAPES[shape]()
    x = perturbed(prob, sigma=2e-2)
    kind = prob[0]
    for face in range(lnp.FACES[kind]):
        fine = lnp.pressure_force(prob, x, face, all_elems(prob), 3e4, 8, 8)
        used = lnp.pressure_force(prob, x, face, all_elems(prob), 3e4)
        scale = np.abs(fine).max()
        err = np.abs(used - fine).max() / scale
        low = 4 if kind == 3443 else 3
        coarse = lnp.pressure_force(prob, x, face, all_elems(prob), 3e4, low, low if kind == 3443 else 2)
        err_low = np.abs(coarse - fine).max() / scale
        print(shape, face, f"kernel rule {err:.2e}  {low}-point rule {err_low:.2e}")
        assert err <= 1e-13
        assert err_low > 1e-10
        if kind == 3243:
            four = lnp.pressure_force(prob, x, face, all_elems(prob), 3e4, 4, 2)
            assert np.abs(four - fine).max() <= 1e-13 * scale


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pressure_on_the_flat_reference_is_minus_p_A_n(shape):
    prob = SHAPES[shape]()
    X = aonp.reference(prob)
    p = 2.5e4
    normals = {3443: [(0, 0, -1), (0, 0, 1)], 3243: [(0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]}[prob[0]]
    for face, n in enumerate(normals):
        f = lnp.pressure_force(prob, X, face, all_elems(prob), p)
        want = -p * face_area(prob, face) * len(all_elems(prob)) * np.array(n, dtype=float)
        assert np.abs(f[0::4].sum(axis=0) - want).max() <= 64 * EPS * np.abs(want).max()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rigid_motion_rotates_pressure_and_leaves_dead_loads(shape):
    prob = SHAPES[shape]()
    x = perturbed(prob)
    xr = x @ Q_ROT.T
    xr[0::4] += np.array([0.3, -1.1, 0.7])                               # the translation moves positions only
    nf = lnp.FACES[prob[0]]
    press = [dict(kind=1, face=f, elems=all_elems(prob), value=3e4 * (f + 1), scale=0.5) for f in range(nf)]
    dead = [dict(kind=0, face=nf - 1, elems=all_elems(prob), value=T_VEC, scale=2.0)]
    f0, f1 = lnp.total(prob, x, RHO, loads=press), lnp.total(prob, xr, RHO, loads=press)
    scale = np.abs(f0).max()
    assert scale > 0 and np.abs(f1 - f0 @ Q_ROT.T).max() <= 1e-12 * scale
    g0, g1 = lnp.total(prob, x, RHO, A_G, dead), lnp.total(prob, xr, RHO, A_G, dead)
    assert np.array_equal(g0, g1) and np.abs(g0).max() > 0


def test_mesh_independence():
    """One element and the refined mesh of the same rectangle / line carrying the same polynomial field: the resultants of
    traction and of pressure agree within 64 EPS x the sum of the absolute terms, the bound of the obstacle tests'
    test_mesh_independence."""
    pairs = [((3443,) + mu.structured_3443_plate(1, 1, 4.0, 2.0) + ((4.0, 2.0, 0.1),),
              (3443,) + mu.structured_3443_plate(2, 2, 2.0, 1.0) + ((2.0, 1.0, 0.1),))]
    gens = []
    for n, L in ((1, 1.0), (2, 0.5)):
        gen = mu.GridMeshGenerator(n * L, 0.0, L, True, False)
        gen.generate_mesh()
        gens.append((3243,) + gen.get_coordinates() + (gen.get_element_connectivity(), (L, 0.1, 0.1)))
    pairs.append(tuple(gens))
    for big, fine in pairs:
        xb = perturbed(big, sigma=2e-2)
        xf = lnp.field_on(big, xb, fine)
        assert np.abs(lnp.field_on(big, xb, big) - xb).max() <= 64 * EPS * np.abs(xb).max()
        for face in range(lnp.FACES[big[0]]):
            for kind, value in ((0, T_VEC), (1, 3e4)):
                ld = lambda prob: [dict(kind=kind, face=face, elems=all_elems(prob), value=value, scale=1.0)]
                fb, ff = lnp.total(big, xb, RHO, loads=ld(big)), lnp.total(fine, xf, RHO, loads=ld(fine))
                rb, rf = fb[0::4].sum(axis=0), ff[0::4].sum(axis=0)
                bound = 64 * EPS * max(np.abs(fb[0::4]).sum(), np.abs(ff[0::4]).sum())
                print(big[0], face, kind, np.abs(rb - rf).max() / bound * 64, "EPS of the sum of the absolute terms")
                assert np.abs(rb - rf).max() <= bound


# ---- surface of the feature -------------------------------------------------------------------------------------------------
def test_symbols_members_and_struct_layout():
    syms = tl.exported_symbols()
    assert all(s in syms for s in NEW)
    assert "SetGravity" in vars(tl.GPU_FEAT10_Data)
    for cls in (tl.GPU_ANCF3243_Data, tl.GPU_ANCF3443_Data):
        assert hasattr(cls, "SetGravity")
        for name in ("AddSurfaceTraction", "AddFollowerPressure", "SetLoadScale", "ClearLoads", "GetLoadForces",
                     "GetLoadResultant"):
            assert name in vars(cls.__mro__[1]), name                    # the ANCF mirror's own
    assert tl.SurfaceTraction and tl.FollowerPressure and "FollowerPressure" in tl.__all__
    # the struct of the header, field by field
    txt = open(tl.binding.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\} tlfea_surface_load;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert decl == ["int kind", "int face", "double value[3]", "double scale", "const int *elems", "int n_elems"]
    S = tl.binding.SurfaceLoadC
    assert [f[0] for f in S._fields_] == ["kind", "face", "value", "scale", "elems", "n_elems"]
    assert (S.kind.offset, S.face.offset, S.value.offset, S.scale.offset, S.elems.offset, S.n_elems.offset) == (0, 4, 8, 32, 40, 48)
    assert C.sizeof(S) == 56
    assert int(re.search(r"#define TLFEA_MAX_LOADS (\d+)", txt).group(1)) == tl.loads.MAX_LOADS == 16


def test_refusals_without_a_gpu():
    """what the mirror refuses before it reaches the C-ABI (which refuses the same again: tests/test_gpu_ancf_loads.py)"""
    shell = tl.GPU_ANCF3443_Data(9, 4)                                   # not initialised: nothing below touches the GPU
    beam = tl.GPU_ANCF3243_Data(3, 2)
    with pytest.raises(ValueError, match="face 2 outside 0..1"):
        shell.AddFollowerPressure(2, [0], 1e4)
    with pytest.raises(ValueError, match="face must be"):
        beam.AddSurfaceTraction(4, [0], T_VEC)
    with pytest.raises(ValueError, match="outside 0..3"):
        shell.AddSurfaceTraction(0, [4], T_VEC)
    with pytest.raises(ValueError, match="negative"):
        shell.AddSurfaceTraction(0, [-1], T_VEC)
    with pytest.raises(ValueError, match="twice"):
        shell.AddFollowerPressure(1, [0, 1, 0], 1e4)
    with pytest.raises(ValueError, match="non-empty"):
        shell.AddFollowerPressure(1, [], 1e4)
    with pytest.raises(ValueError, match="finite"):
        shell.AddFollowerPressure(1, [0], float("nan"))
    with pytest.raises(ValueError, match="3-vector"):
        shell.AddSurfaceTraction(1, [0], [1.0, 2.0])
    shell._loads = [tl.FollowerPressure(1, [0], 1.0)] * 16
    with pytest.raises(ValueError, match="at most 16"):
        shell.AddFollowerPressure(1, [0], 1e4)
    with pytest.raises(ValueError, match="outside the 16"):
        shell.SetLoadScale(16, 1.0)
    with pytest.raises(ValueError, match="3-vector"):
        shell.SetGravity([0.0, 1.0])
    assert not hasattr(tl.GPU_FEAT10_Data, "AddSurfaceTraction")        # surface loads are not offered on T10


def test_inflation_driver_builds(tmp_path):
    lib_dir = os.path.join(ROOT, "total-lagrangian-fea_amd")
    out = tmp_path / "test_shell_inflation"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(out),
                           os.path.join(HOST, "test_shell_inflation.cc"), "-L" + lib_dir, "-ltlfea_hip",
                           "-Wl,-rpath," + lib_dir])
    assert out.exists()
