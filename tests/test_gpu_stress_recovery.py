"""The recovered stress on the GPU (DESIGN 3f''), through the Python mirror: the kernels against tests/stress_recovery_np.py
fed with the GPU's own point stresses, exactness on a linear field through the point hook, the principal stresses at
simple, multiple and nearly multiple roots, reproducibility, no disturbance of the stress recovery or of a step, the
refusals and the mesh-sequence driver."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests import stress_np as snp
from tests import stress_recovery_np as rnp
from tests.helpers import MATERIALS, load_mesh, make_gpu, perturbed_state
from tests.test_gpu_adjoint import set_table, table_of
from tests.test_gpu_stress import cantilever, move
from tests.test_stress import Q_ROT
from tests.test_stress_recovery_np import linear_field, linear_points

tl = importlib.import_module("total-lagrangian-fea_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
BARY = tl.quadrature.tet5pt_bary
QW = tl.quadrature.tet5pt_weights
T, NQ = rnp.table(BARY), rnp.shape_at_points(BARY)


def retrieved(d, directions=True):
    n, p, (eta2, n2), est = (d.RetrieveRecoveredStressToCPU(), d.RetrievePrincipalStressToCPU(directions=directions),
                             d.RetrieveErrorIndicatorToCPU(), d.GetErrorEstimate())
    return dict(nodal_sigma=n.sigma, nodal_von_mises=n.von_mises, nodal_principal=p.nodal_values, nodal_tau=p.nodal_tau_max,
                elem_principal=p.element_values, elem_tau=p.element_tau_max, nodal_dir=p.nodal_directions,
                elem_dir=p.element_directions, eta2=eta2, n2=n2, eta2_total=est.eta2, n2_total=est.n2, eta_rel=est.eta_rel,
                clamped=est.clamped)


def restated(d, pts, mu, K):
    conn, detJ = d.RetrieveConnectivityToCPU(), d.RetrieveDetJToCPU()
    nod = rnp.recovered_nodal(pts, detJ, QW, conn, d.get_n_coef(), T)
    out = rnp.error_indicator(pts, nod, detJ, QW, conn, NQ, mu, K)
    pn, tn, _ = rnp.principal(nod)
    pe, te, _ = rnp.principal(rnp.element_mean(pts, detJ, QW))
    out.update(nodal_sigma=nod, nodal_von_mises=snp.von_mises(nod), nodal_principal=pn, nodal_tau=tn, elem_principal=pe,
               elem_tau=te)
    return out


FIELDS = ("nodal_sigma", "nodal_von_mises", "nodal_principal", "nodal_tau", "elem_principal", "elem_tau", "eta2", "n2")
TOTALS = ("eta2_total", "n2_total", "eta_rel")


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------
CASES = [(tag, mat) for tag in ("cube", "beam_3x2x1", "res2") for mat in ("svk", "mr", "table")] + [("res2", "svk_damped+v")]


@pytest.mark.parametrize("tag,mat", CASES)
def test_kernels_against_restatement(tag, mat):
    X, conn = load_mesh(tag)
    x, v = perturbed_state(X)
    with_v = mat.endswith("+v")
    kind = "svk" if mat == "table" else mat.split("+")[0]
    m = MATERIALS[kind]
    d = make_gpu(X, conn, m)
    mu, K = rnp.moduli(m)
    if mat == "table":
        mats, ids = table_of("svk"), (np.arange(conn.shape[0]) % 3).astype(np.int32)
        set_table(d, "svk", mats, ids)
        mk = np.array([rnp.moduli(dict(kind="svk", **e)) for e in mats])
        mu, K = mk[ids, 0], mk[ids, 1]
    move(d, x)
    d.CalcStress(v if with_v else None, points=True)
    d.RecoverStress(principal=True, directions=True)
    got, ref = retrieved(d), restated(d, d.RetrievePointStressToCPU(), mu, K)
    for name in FIELDS:
        scale = np.abs(ref[name]).max()
        err = np.abs(got[name] - ref[name]).max()
        print(f"{tag} {mat} {name}: {err / scale:.2e}")
        assert err <= 1e-10 * scale, name
    for name in TOTALS:
        print(f"{tag} {mat} {name}: {got[name]:.15e} vs {ref[name]:.15e}")
        assert abs(got[name] - ref[name]) <= 1e-12 * abs(ref[name]), name
    assert got["clamped"] == ref["clamped"]
    assert np.array_equal(got["eta2"] >= 0, np.ones(conn.shape[0], dtype=bool))
    f = d.size_factors(0.05)
    assert np.array_equal(f, tl.size_factors(got["eta2"], got["n2"], 0.05)) and f.min() >= 0.25 and f.max() <= 4.0
    assert d.GetRecoveredStressDevicePtr()
    d.Destroy()


# ---- 2. exactness through the point hook -------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["beam_3x2x1", "res2"])
def test_linear_field_through_the_point_hook(tag):
    X, conn = load_mesh(tag)
    d = make_gpu(X, conn, MATERIALS["svk"])
    d.RecoverStressFromPoints(linear_points(X, conn))             # no CalcStress before it
    want = linear_field(X)
    got = retrieved(d, directions=False)
    err = np.abs(got["nodal_sigma"] - want).max() / np.abs(want).max()
    print(f"{tag}: nodal error {err:.3e} of the largest entry, eta_rel {got['eta_rel']:.3e}")
    assert err <= 1e-12
    assert got["eta_rel"] <= 1e-12
    d.Destroy()


# ---- 3. principal stresses ---------------------------------------------------------------------------------------------
GENERAL = np.array([4.0e6, -1.5e6, 2.5e6, 1.2e6, -0.8e6, 0.6e6])
TENSORS = {
    "zero": np.zeros(6),
    "hydrostatic": np.array([-2.0e6, -2.0e6, -2.0e6, 0.0, 0.0, 0.0]),
    "uniaxial": np.array([5.0e6, 0.0, 0.0, 0.0, 0.0, 0.0]),
    "pure_shear": np.array([0.0, 0.0, 0.0, 3.0e6, 0.0, 0.0]),
    "general": GENERAL,
    "near_double": snp.voigt(Q_ROT @ np.diag([1.0e6, 1.0e6 * (1.0 + 1e-9), -0.5e6]) @ Q_ROT.T),
    "general_1e12": GENERAL * 1e12,
    "general_1e-6": GENERAL * 1e-6,
}


@pytest.fixture(scope="module")
def cube_object():
    X, conn = load_mesh("cube")
    d = make_gpu(X, conn, MATERIALS["svk"])
    yield d
    d.Destroy()


@pytest.mark.parametrize("name", list(TENSORS))
def test_principal_stresses(cube_object, name):
    d, s6 = cube_object, TENSORS[name]
    E = d.RetrieveConnectivityToCPU().shape[0]
    d.RecoverStressFromPoints(np.broadcast_to(s6, (E, 5, 6)).copy(), principal=True, directions=True)
    p = d.RetrievePrincipalStressToCPU(directions=True)
    nodal = d.RetrieveRecoveredStressToCPU().sigma
    frob = np.sqrt((snp.tensor(s6) ** 2).sum())
    w = np.linalg.eigvalsh(snp.tensor(s6))[::-1]
    for where, sig, val, tau, vec in (("nodal", nodal, p.nodal_values, p.nodal_tau_max, p.nodal_directions),
                                      ("element", np.broadcast_to(s6, (E, 6)), p.element_values, p.element_tau_max,
                                       p.element_directions)):
        S = snp.tensor(sig)
        gap = np.abs(val - w).max()
        res = np.linalg.norm(np.einsum("nij,nkj->nki", S, vec) - val[:, :, None] * vec, axis=2).max()
        orth = np.abs(vec @ np.swapaxes(vec, 1, 2) - np.eye(3)).max()
        det = np.linalg.det(vec)
        print(f"{name} {where}: eigenvalue gap {gap:.2e}, residual {res:.2e} (|sigma|_F {frob:.2e}), orthonormality {orth:.2e}")
        assert gap <= 1e-10 * frob
        assert np.all(val[:, 0] >= val[:, 1]) and np.all(val[:, 1] >= val[:, 2])
        assert np.array_equal(tau, 0.5 * (val[:, 0] - val[:, 2]))
        assert res <= 1e-10 * frob
        assert orth <= 1e-12
        assert np.abs(det - 1.0).max() <= 1e-12


# ---- 4. reproducibility, nothing disturbed -----------------------------------------------------------------------------
def test_reproducible_and_leaves_the_stress_recovery_alone():
    X, conn = load_mesh("res2")
    m = MATERIALS["mr"]
    x, _ = perturbed_state(X)
    runs = []
    for _ in range(2):
        d = make_gpu(X, conn, m)
        move(d, x)
        d.CalcStress(points=True)
        before = (d.RetrieveNodalStressToCPU(), d.RetrieveElementStressToCPU(), d.GetEnergies())
        for _ in range(2):
            d.RecoverStress(principal=True, directions=True)
            r = retrieved(d)
            runs.append([np.asarray(r[k]) for k in sorted(r)])
        after = (d.RetrieveNodalStressToCPU(), d.RetrieveElementStressToCPU(), d.GetEnergies())
        for a, b in zip(before, after):
            for fa, fb in zip(a, b):
                assert np.array_equal(np.asarray(fa), np.asarray(fb))
        d.Destroy()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b)


def test_does_not_disturb_a_step():
    out = []
    for with_recovery in (False, True):
        X, d, s, _, _ = cantilever("res2")
        for _ in range(3):
            s.Solve()
            if with_recovery:
                d.CalcStress(points=True)
                d.RecoverStress()
        out.append((np.stack(d.RetrievePositionToCPU()), s.RetrieveVelocityToCPU()))
        del s
        d.Destroy()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def refused(call, text):
    with pytest.raises(tl.TlfeaError) as e:
        call()
    assert str(e.value) == text


def test_refusals():
    B = importlib.import_module("total-lagrangian-fea_amd.binding")
    lib = tl.load_library()
    X, conn = load_mesh("beam_3x2x1")
    q = tl.quadrature
    d = tl.GPU_FEAT10_Data(conn.shape[0], X.shape[0])
    d.Initialize()
    d.Setup(q.tet5pt_x, q.tet5pt_y, q.tet5pt_z, q.tet5pt_weights, X[:, 0], X[:, 1], X[:, 2], conn)
    d.SetDensity(1000.0)
    d.SetSVK(1e7, 0.3)
    pts = np.zeros((conn.shape[0], 5, 6))
    refused(lambda: d.RecoverStressFromPoints(pts), "tlfea_t10_recover_stress_from_points: CalcDnDuPre must be called first")
    d.CalcDnDuPre()
    refused(d.RecoverStress, "tlfea_t10_recover_stress: tlfea_t10_calc_stress has not been called")
    for call, name in ((d.RetrieveRecoveredStressToCPU, "retrieve_recovered_stress"),
                       (d.RetrievePrincipalStressToCPU, "retrieve_principal_stress"),
                       (d.RetrieveErrorIndicatorToCPU, "retrieve_error_indicator"), (d.GetErrorEstimate, "get_error_estimate")):
        refused(call, f"tlfea_t10_{name}: tlfea_t10_recover_stress has not been called")
    assert not d.GetRecoveredStressDevicePtr()
    d.CalcStress()
    refused(d.RecoverStress, "tlfea_t10_recover_stress: the last tlfea_t10_calc_stress did not ask for point stresses "
                             "(want_points = 0)")
    refused(lambda: d.TimeRecoveryKernels(1), "tlfea_t10_time_recovery_kernels: the last tlfea_t10_calc_stress did not ask "
                                              "for point stresses (want_points = 0)")
    d.CalcStress(points=True)
    d.RecoverStress(principal=False)
    refused(d.RetrievePrincipalStressToCPU, "tlfea_t10_retrieve_principal_stress: the last tlfea_t10_recover_stress did not "
                                            "compute principal stresses (want_principal = 0)")
    d.RecoverStress(principal=True)
    d.RetrievePrincipalStressToCPU()
    refused(lambda: d.RetrievePrincipalStressToCPU(directions=True),
            "tlfea_t10_retrieve_principal_stress: the last tlfea_t10_recover_stress did not compute principal directions "
            "(want_directions = 0)")
    # null outputs and inputs
    h = d._h
    assert lib.tlfea_t10_get_error_estimate(h, None) != 0
    assert lib.tlfea_last_error().decode() == "tlfea_t10_get_error_estimate: null output"
    assert lib.tlfea_t10_recover_stress_from_points(h, None, 1, 0) != 0
    assert lib.tlfea_last_error().decode() == "tlfea_t10_recover_stress_from_points: null points"
    assert lib.tlfea_t10_time_recovery_kernels(h, 1, None) != 0
    assert lib.tlfea_last_error().decode() == "tlfea_t10_time_recovery_kernels: null output"
    d.RecoverStress()                                                # the refused calls left the object usable
    assert lib.tlfea_t10_retrieve_recovered_stress(h, None, None) == 0   # null = not wanted
    assert lib.tlfea_t10_retrieve_principal_stress(h, None, None, None, None) == 0
    assert lib.tlfea_t10_retrieve_error_indicator(h, None, None) == 0
    with pytest.raises(ValueError, match="entries"):
        d.RecoverStressFromPoints(np.zeros(7))
    d.Destroy()
    a = tl.GPU_ANCF3243_Data(2, 1)
    a.Initialize()
    buf = np.zeros(64)
    not_ancf = ": T10 handles only (not an ANCF handle)"
    for name, args in (("recover_stress", (1, 0)), ("recover_stress_from_points", (B.dp(buf), 1, 0)),
                       ("retrieve_recovered_stress", (B.dp(buf), B.dp(buf))),
                       ("retrieve_principal_stress", (B.dp(buf), None, B.dp(buf), None)),
                       ("retrieve_error_indicator", (B.dp(buf), B.dp(buf))), ("get_error_estimate", (B.dp(buf),)),
                       ("time_recovery_kernels", (1, B.dp(buf)))):
        assert getattr(lib, "tlfea_t10_" + name)(a._h, *args) != 0, name
        assert lib.tlfea_last_error().decode() == "tlfea_t10_" + name + not_ancf
    assert not lib.tlfea_t10_recovered_stress_device_ptr(a._h)
    a.Destroy()


# ---- 6. driver ---------------------------------------------------------------------------------------------------------
def test_beam_error_driver(tmp_path):
    exe = os.path.join(HOST, "test_beam_error")
    assert os.path.exists(exe), "build the host drivers first (make -C total-lagrangian-fea_amd/host)"
    vtu = tmp_path / "beam_error.vtu"
    p = subprocess.run(["timeout", "-k", "10", "300", exe, "--mesh_dir=" + os.path.join(ROOT, "tests", "golden", "meshes"),
                        "--vtu=" + str(vtu), "beam_3x2x1_res2.1", "beam_3x2x1_res4.1"], capture_output=True, text=True,
                       timeout=320)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [ln for ln in p.stdout.splitlines() if ln.startswith("Mesh ")]
    assert len(rows) == 2
    elems = [int(re.search(r"elements=(\d+)", r).group(1)) for r in rows]
    eta = [float(re.search(r"eta_rel=(\S+)", r).group(1)) for r in rows]
    assert elems == [199, 936]
    assert 0.0 < eta[1] < eta[0] < 1.0
    for r in rows:
        assert float(re.search(r"max_von_mises=(\S+)", r).group(1)) > 0.0
        assert 0.25 <= float(re.search(r"median_size_factor=(\S+)", r).group(1)) <= 4.0
    txt = vtu.read_text()
    n = int(re.search(r'NumberOfPoints="(\d+)"', txt).group(1))
    for name, comps, count in (("stress", 6, n), ("von_mises", 1, n), ("principal", 3, n), ("eta", 1, 936)):
        body = re.search(r'<DataArray type="Float64" Name="%s"[^>]*>\n(.*?)</DataArray>' % name, txt, re.S).group(1)
        lines = [ln for ln in body.splitlines() if ln.strip()]
        assert len(lines) == count and all(len(ln.split()) == comps for ln in lines), name
    assert txt.index("<CellData>") < txt.index('Name="eta"') < txt.index("</CellData>")
