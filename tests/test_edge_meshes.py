"""The meshes of tests/edge_meshes.py, checked without a GPU: the counts each builder promises, det J > 0 in every element
(the CPU oracle's), the largest LDS accumulator the row-group builders report for the hub of the stars -- and that the
judge of tests/test_gpu_elem_forms.py rejects an H that is wrong in the ways an assembly kernel can be wrong.  (The
row-group invariants themselves run on these meshes in tests/test_rowgroups.py.)"""
import numpy as np
import pytest

from tests import edge_meshes as em
from tests import elem_forms_worker as w
from tests.helpers import MATERIALS, make_oracle
from tests.test_rowgroups import adjacency, dp, ip, shim  # noqa: F401  (shim: the fixture)

mu = em.mu


@pytest.mark.parametrize("name", sorted(em.COUNTS))
def test_counts_and_orientation(name):
    X, conn = em.build(name)
    N, E, maxdeg = em.COUNTS[name]
    assert X.shape == (N, 3) and X.dtype == np.float64 and conn.shape == (E, 10) and conn.dtype == np.int32
    assert conn.min() >= 0 and conn.max() < N
    for k, (a, b) in enumerate(mu.EDGES):                     # mid-edge nodes in the standard order, on their edges
        assert np.allclose(X[conn[:, 4 + k]], 0.5 * (X[conn[:, a]] + X[conn[:, b]]), atol=1e-15)
    o = make_oracle(X, conn, MATERIALS["svk"])
    assert o.detJ.min() > 0
    assert int(np.diff(o.m_off).max()) == maxdeg
    unused = np.setdiff1d(np.arange(N), conn)
    if name == "isolated_box":
        assert np.array_equal(unused, em.isolated_box()[2]) and unused.tolist() == [0, 37, 77]
        assert np.all(np.diff(o.m_off)[unused] == 0)           # empty rows, no diagonal entry
        ro, _ = o.hessian_pattern()
        assert np.all(np.diff(ro).reshape(N, 3)[unused] == 0)
    else:
        assert unused.size == 0                                # box_65 / box_63 included: no node is isolated


def test_special_nodes():
    for nsub in (2, 3):
        X, conn = em.star(nsub)
        hub = em.star_hub(X, conn)
        assert hub == conn[:, :4].max() and np.all(X[hub] == 0.0)      # the last vertex, before every mid-edge node
        assert hub + 1 == conn[:, 4:].min()
    X, conn = em.build("box_65")
    assert conn.shape[0] % 64 == 1 and em.build("box_63")[1].shape[0] % 64 == 63 and em.build("box_192")[1].shape[0] % 64 == 0
    Xc, _ = em.build("curved_star2")
    moved = np.where(np.any(Xc != em.build("star2")[0], axis=1))[0]
    assert moved.tolist() == [int(em.build("star2")[1][0, 4])]
    assert make_oracle(Xc, em.build("star2")[1], MATERIALS["svk"]).detJ.min() > 0


@pytest.mark.parametrize("name", sorted(em.STAR_ACC_MAX))
def test_star_accumulators(shim, name):  # noqa: F811
    """acc_max of both row-group forms: 9 doubles per block of the hub's row (star4: the builders accept it -- 16-bit
    packing -- although 46 125 doubles are 360 KiB; the solver's set-up refuses it by the device's LDS limit)"""
    X, conn = em.build(name)
    N, (E, S) = X.shape[0], conn.shape
    off, cols, n2e_off, n2e = adjacency(conn, N)
    conn_cm = np.ascontiguousarray(conn.T)
    x, y, z = (np.ascontiguousarray(X[:, k]) for k in range(3))
    sizes = np.zeros(5, dtype=np.int32)
    assert shim.rg_build(N, E, S, ip(conn_cm), ip(off), ip(cols), ip(n2e_off), ip(n2e), dp(x), dp(y), dp(z), ip(sizes)) == 0
    assert int(sizes[2]) == em.STAR_ACC_MAX[name]
    sizes4 = np.zeros(4, dtype=np.int32)
    assert shim.rg4_build(N, E, ip(conn_cm), ip(off), ip(cols), ip(n2e_off), ip(n2e), dp(x), dp(y), dp(z), ip(sizes4)) == 0
    assert int(sizes4[2]) == em.STAR_ACC_MAX[name]
    assert em.STAR_ACC_MAX == {"star2": 2925, "star3": 11565, "star4": 46125, "cone_22x20": 19845}


# ---- the judge can fail ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star2_reference():
    c = w.case("star2", "svk", hub_pinned=True)
    inp = w.case_inputs(c)
    ref = w.oracle_reference(inp)
    o = make_oracle(inp["X"], inp["conn"], inp["material"], inp["fixed"])
    o.x, o.y, o.z = (np.ascontiguousarray(inp["x"][:, i]) for i in range(3))
    Ke, _ = o.element_tangents()
    return inp, ref, Ke, em.star_hub(inp["X"], inp["conn"])


def block_slots(ref, i, j):
    """indices into the CSR values of the 3 x 3 block (node row i, node column j): [3, 3]"""
    ro, ci = ref["ro"], ref["ci"]
    out = np.zeros((3, 3), dtype=np.int64)
    for d in range(3):
        row = ci[ro[3 * i + d]:ro[3 * i + d + 1]]
        k = int(np.searchsorted(row, 3 * j))
        assert row[k] == 3 * j
        out[d] = ro[3 * i + d] + k + np.arange(3)
    return out


def judged(inp, ref, val):
    return w.judge_hessian(inp["X"].shape[0], ref["ro"], ref["ci"], val, ref["ro"], ref["ci"], ref["val"], val, "star2")


def test_judge_accepts_the_oracle(star2_reference):
    inp, ref, _, _ = star2_reference
    assert judged(inp, ref, ref["val"].copy()) == 0.0


def test_judge_rejects_a_missing_element_contribution(star2_reference):
    inp, ref, Ke, hub = star2_reference
    e = 17
    a = int(np.where(inp["conn"][e] == hub)[0][0])
    val = ref["val"].copy()
    for b, j in enumerate(inp["conn"][e]):                     # h K_e(hub, j) leaves the hub row
        val[block_slots(ref, hub, int(j))] -= w.H_STEP * Ke[e][3 * a:3 * a + 3, 3 * b:3 * b + 3]
    assert w.relerr(val, ref["val"]) > 1e-6
    with pytest.raises(AssertionError):
        judged(inp, ref, val)


def test_judge_rejects_a_doubled_mass_block(star2_reference):
    inp, ref, _, hub = star2_reference
    j = int(inp["conn"][5, 7])
    k = ref["m_off"][hub] + int(np.searchsorted(ref["m_col"][ref["m_off"][hub]:ref["m_off"][hub + 1]], j))
    assert ref["m_col"][k] == j and ref["m_val"][k] != 0.0
    val = ref["val"].copy()
    val[np.diag(block_slots(ref, hub, j))] += ref["m_val"][k] / w.H_STEP
    with pytest.raises(AssertionError):
        judged(inp, ref, val)


def test_judge_rejects_a_penalty_on_the_next_row(star2_reference):
    inp, ref, _, hub = star2_reference
    assert hub in inp["fixed"] and hub + 1 not in inp["fixed"]
    val = ref["val"].copy()
    pen = w.H_STEP * w.H_STEP * w.RHO
    val[np.diag(block_slots(ref, hub, hub))] -= pen
    val[np.diag(block_slots(ref, hub + 1, hub + 1))] += pen
    with pytest.raises(AssertionError):
        judged(inp, ref, val)


def test_judge_rejects_a_row_shifted_by_one_block(star2_reference):
    inp, ref, _, hub = star2_reference
    val = ref["val"].copy()
    r = 3 * hub + 1
    val[ref["ro"][r]:ref["ro"][r + 1]] = np.roll(val[ref["ro"][r]:ref["ro"][r + 1]], 3)
    with pytest.raises(AssertionError):
        judged(inp, ref, val)
