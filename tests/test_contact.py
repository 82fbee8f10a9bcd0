"""Contact subsystem without a GPU: the NumPy restatement of the narrowphase (tests/contact_np.py) on hand-built tet
pairs with closed-form answers, the .npz scalar-field loaders of the Python and C++ MeshManager, and the C++ facade."""
import os
import subprocess

import numpy as np
import pytest

from tests import contact_np as cnp
from tests.helpers import MESHES, tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
SPHERE = os.path.join(MESHES, "sphere.1")
NPZ = os.path.join(MESHES, "sphere.1.uncompressed.npz")
UNIT = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])


def field(v, a, b):
    return v @ np.asarray(a, dtype=float) + b


def test_plane_cuts_unit_tet_in_a_triangle_and_a_quad():
    n = np.array([0.0, 0, 1])
    tri = cnp.plane_tet(UNIT, n, -0.5)            # z = 1/2: triangle with legs 1/2
    assert len(tri) == 3
    area, cen = cnp.area_centroid(tri)
    assert abs(area - 0.125) < 1e-15 and np.allclose(cen, [1 / 6, 1 / 6, 0.5], atol=1e-15)
    n2 = np.array([1.0, 1, 0])
    quad = cnp.plane_tet(UNIT, n2, -0.5)          # x + y = 1/2 splits {0, 3} from {1, 2}: a quad
    assert len(quad) == 4
    area, _ = cnp.area_centroid(quad)
    # vertices (1/2,0,0) (0,1/2,0) (0,1/2,1/2) (1/2,0,1/2): a rectangle sqrt(2)/2 x 1/2
    assert abs(area - np.sqrt(2) / 4) < 1e-15


def test_clipping_yields_three_to_eight_vertices():
    z0 = lambda pts: [np.array([x, y, 0.0]) for x, y in pts]  # noqa: E731
    tri = z0([(0, 0), (1, 0), (0, 1)])
    # a tet much larger than the triangle keeps it whole
    big = np.array([[-5.0, -5, -5], [20, -5, -5], [-5, 20, -5], [-5, -5, 20]])
    assert len(cnp.clip_tet(tri, big)) == 3
    # a tet whose z = 0 section is the triangle mirrored through its centroid: the star's hexagon, 2/3 of the area
    c = np.array([1 / 3, 1 / 3, 0.0])
    S = [2 * c - t for t in tri]
    star = np.array([c + 2 * (s - c) - [0, 0, 1] for s in S] + [c + [0, 0, 1]])
    hexa = cnp.clip_tet(tri, star)
    area, cen = cnp.area_centroid(hexa)
    assert len(hexa) == 6 and abs(area - 1 / 3) < 1e-15 and np.allclose(cen, c, atol=1e-15)
    # a tet whose z = 0 section is the diamond |x| + |y| <= 3/2: it cuts the 4 corners of [-1, 1]^2 -> an octagon
    sq = z0([(-1, -1), (1, -1), (1, 1), (-1, 1)])
    a = 1.5
    dia = np.array([[a, a, -1], [-a, -a, -1], [a, -a, 1], [-a, a, 1]])
    octa = cnp.clip_tet(sq, dia)
    area, cen = cnp.area_centroid(octa)
    assert len(octa) == 8 and abs(area - 3.5) < 1e-14 and np.allclose(cen, 0, atol=1e-15)


def test_equal_plane_patch_between_overlapping_tets():
    """Two unit tets with p_A = 1 - z, p_B = 2 z: the plane 1 - z = 2 z at z = 1/3 inside both."""
    vA, vB = UNIT, UNIT.copy()
    pt = cnp.patch(vA, field(vA, [0, 0, -1], 1.0), vB, field(vB, [0, 0, 2], 0.0))
    assert pt["isValid"] and pt["validOrientation"]
    assert np.allclose(pt["normal"], [0, 0, 1]) and abs(pt["p_equilibrium"] - 2 / 3) < 1e-15
    assert abs(pt["area"] - 0.5 * (2 / 3) ** 2) < 1e-15
    assert abs(pt["g_A"] - 1) < 1e-15 and abs(pt["g_B"] - 2) < 1e-15
    F, wA, wB = cnp.patch_force(pt, vA, vB)
    assert np.allclose(F, [0, 0, 2 / 3 * pt["area"]]) and abs(wA.sum() - 1) < 1e-15 and np.allclose(wA, wB)


def test_parallel_fields_and_degenerate_tets_are_skipped():
    vA = UNIT
    assert not cnp.patch(vA, field(vA, [0, 0, 1], 0.0), vA, field(vA, [0, 0, 1], 0.5))["isValid"]  # n = 0
    flat = UNIT.copy()
    flat[3] = [0.3, 0.3, 0.0]
    assert cnp.affine_fit(flat, np.ones(4)) is None
    assert not cnp.patch(flat, np.arange(4.0), vA, field(vA, [0, 0, 1], 0.0))["isValid"]


def test_orientation_flip_and_invalid_orientation():
    vA = vB = UNIT
    # A's pressure grows upwards, B's downwards: n = aA - aB points up, g_A < 0 -> flipped to point down
    pt = cnp.patch(vA, field(vA, [0, 0, 2], 0.0), vB, field(vB, [0, 0, -1], 1.0))
    assert pt["isValid"] and pt["validOrientation"] and np.allclose(pt["normal"], [0, 0, -1])
    assert pt["g_A"] > 0 and pt["g_B"] > 0
    # both fields grow upwards at different rates: no direction makes both gradients positive
    pt = cnp.patch(vA, field(vA, [0, 0, 2], -0.5), vB, field(vB, [0, 0, 1], 0.0))
    assert pt["isValid"] and not pt["validOrientation"]
    assert cnp.patch_force(pt, vA, vB)[0] is None


def two_sphere_manager():
    mm = tl.MeshManager()
    for _ in range(2):
        assert mm.LoadMesh(SPHERE + ".node", SPHERE + ".ele") >= 0
    return mm


def test_python_npz_loader_scatters_through_original_vertex_ids():
    mm = two_sphere_manager()
    assert mm.LoadScalarFieldFromNpz(0, NPZ)
    f = mm.GetAllScalarFields()
    z = np.load(NPZ)
    assert z["original_vertex_ids"].min() == 1 and f.size == 2 * 529
    assert np.array_equal(f[:95], z["p_vertex"]) and not np.any(f[95:])
    assert np.any(f[:95] > 0)
    assert mm.LoadScalarFieldFromNpz(1, NPZ) and np.array_equal(mm.GetAllScalarFields()[529:529 + 95], z["p_vertex"])
    assert not mm.LoadScalarFieldFromNpz(0, NPZ, "no_such_key")
    assert list(np.unique(mm.GetAllElementMeshIds())) == [0, 1]


def build_host(target):
    subprocess.check_call(["make", "-C", HOST, target], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, target)


def test_cpp_npz_loader_matches_python_and_refuses_compressed(tmp_path):
    exe = build_host("check_npz_field")
    out = subprocess.run([exe, f"--mesh={SPHERE}", f"--npz={NPZ}"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    mm = two_sphere_manager()
    assert mm.LoadScalarFieldFromNpz(0, NPZ)
    assert np.array_equal(np.array(out.stdout.split(), dtype=float), mm.GetAllScalarFields())
    z = np.load(NPZ)
    comp = tmp_path / "compressed.npz"
    np.savez_compressed(comp, p_vertex=z["p_vertex"], original_vertex_ids=z["original_vertex_ids"])
    bad = subprocess.run([exe, f"--mesh={SPHERE}", f"--npz={comp}"], capture_output=True, text=True)
    assert bad.returncode == 2 and "compressed" in bad.stderr
    f32 = tmp_path / "float32.npz"
    np.savez(f32, p_vertex=z["p_vertex"].astype(np.float32), original_vertex_ids=z["original_vertex_ids"])
    bad = subprocess.run([exe, f"--mesh={SPHERE}", f"--npz={f32}"], capture_output=True, text=True)
    assert bad.returncode == 2 and "dtype" in bad.stderr
    i32 = tmp_path / "int32_ids.npz"
    np.savez(i32, p_vertex=z["p_vertex"], original_vertex_ids=z["original_vertex_ids"].astype(np.int32))
    bad = subprocess.run([exe, f"--mesh={SPHERE}", f"--npz={i32}"], capture_output=True, text=True)
    assert bad.returncode == 2 and "original_vertex_ids" in bad.stderr and "dtype" in bad.stderr
    assert subprocess.run([exe, "--bogus"], capture_output=True).returncode == 1


def test_sphere_drop_driver_builds_with_gxx_and_rejects_unknown_flags():
    exe = build_host("test_sphere_drop_collision")
    r = subprocess.run([exe, "--bogus"], capture_output=True, text=True)
    assert r.returncode == 1 and "--bogus" in r.stderr


def test_collision_facade_compiles_with_plain_gxx(tmp_path):
    src = tmp_path / "use_collision.cc"
    src.write_text('#include "tlfea_collision.h"\n'
                   "int main() {\n"
                   "  CollisionSystemParams p{0.2, 0.8};\n"
                   "  CollisionSystemInput in;\n"
                   "  HydroelasticPatchCollisionSystem* c = nullptr;\n"
                   "  if (c) { c->Step(in, p); c->ApplyToElementData(); (void)c->GetValidPatches(); }\n"
                   "  return p.damping > 0 ? 0 : 1;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{HOST}", str(src)])
