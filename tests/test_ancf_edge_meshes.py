"""The meshes of tests/ancf_edge_meshes.py, checked without a GPU: the counts each builder promises, the length of the hub's
row and the LDS it needs in assemble_rows_kernel against what the configurations of tests/ancf_forms_worker.py expect, det J
> 0 at every force and mass point (the CPU oracle's), a positive diagonal of the mass matrix -- and that the judge of
tests/test_gpu_ancf_forms.py rejects an H that is wrong in the ways the two kernels can be wrong."""
import numpy as np
import pytest

from tests import ancf_edge_meshes as am
from tests import ancf_forms_worker as w


def detj_at(inp, rule):
    """det J of the oracle at the points of its 'force_rule' or 'mass_rule'"""
    o = w.make_oracle(inp)
    if rule == "mass_rule":
        o.force_rule = o.mass_rule
        nq = len(o.mass_rule[0]) * len(o.mass_rule[1]) * len(o.mass_rule[2])
        o.gradN, o.detJ = np.zeros((o.E, nq, 3, o.S)), np.zeros((o.E, nq))
        o.calc_dsdu_pre()
    return o.detJ.copy(), o


@pytest.mark.parametrize("name", sorted(am.COUNTS))
def test_counts_orientation_and_mass(name):
    m = am.build(name)
    kind, x, y, z, conn, L, W, H = m
    N, E, longest = am.COUNTS[name]
    nn = {3243: 2, 3443: 4}[kind]
    assert len(x) == len(y) == len(z) == N and N % 4 == 0 and conn.shape == (E, nn) and conn.dtype == np.int32
    assert L.shape == W.shape == H.shape == (E,) and conn.min() >= 0 and conn.max() < N // 4
    assert am.hub_row_blocks(m) == longest and am.assemble_rows_lds_bytes(m) == 72 * longest
    inp = w.case_inputs(w.case(name, "svk"))
    for rule in ("force_rule", "mass_rule"):
        detJ, o = detj_at(inp, rule)
        assert detJ.shape[0] == E and detJ.min() > 0, (name, rule, detJ.min())
    o = w.make_oracle(inp)
    assert int(np.diff(o.m_off).max()) == longest
    unused = am.unused_nodes(m)
    rows = np.diff(o.m_off).reshape(-1, 4)
    if name.startswith("isolated_"):
        assert unused.tolist() == [N // 4 - 2, N // 4 - 1] and np.all(rows[unused] == 0)      # four empty coefficient rows each
        assert set(am.node_coefficients(unused[0])) <= set(inp["fixed"].tolist())             # one of them pinned
        assert not set(am.node_coefficients(unused[1])) & set(inp["fixed"].tolist())
        ro, _ = o.hessian_pattern()
        assert np.all(np.diff(ro).reshape(-1, 12)[unused] == 0)
    else:
        assert unused.size == 0
    used = np.setdiff1d(np.arange(N // 4), unused)
    M = o.mass_dense()
    assert np.all(np.diag(M)[am.node_coefficients(used)] > 0)
    if name.startswith("graded_"):
        base = am.build(name[len("graded_"):])
        assert all(np.array_equal(a, b) for a, b in zip(m[1:5], base[1:5]))                   # positions are not moved
        assert len(np.unique(L)) == E and len(np.unique(detj_at(inp, "force_rule")[0][:, 0])) == E


def test_fans():
    for k in (8, 9, 230):
        m = am.fan3243(k)
        assert am.hub_row_blocks(m) == 4 + 4 * k and w.hub_of(m[4]) == 0 and np.all(m[4][:, 0] == 0)
        tips = np.stack([m[1][4::4], m[2][4::4], m[3][4::4]], axis=1)
        assert np.allclose(np.linalg.norm(tips, axis=1), am.BEAM_DIMS[0], atol=1e-15)
        assert np.all(tips[:, 0] / am.BEAM_DIMS[0] >= np.cos(am.CAP_HALF_ANGLE))
        assert len(np.unique(np.round(tips, 12), axis=0)) == k
    for k in (8, 9, 80):
        m = am.fan3443(k)
        assert am.hub_row_blocks(m) == 4 + 12 * k and w.hub_of(m[4]) == 0 and np.all(m[4][:, 0] == 0)
        assert len(np.unique(m[4][:, 1:])) == 3 * k                                           # three nodes of its own per shell
        assert np.abs(m[3][4::4]).max() <= 0.1                                                # the lift in z
    # chunks of 8 incident elements in the hub's row (assemble_rows_kernel): whole chunks and the elements of the last one
    chunks = {name: divmod(int(np.sum(am.build(name)[4] == 0)), 8) for name in am.COUNTS if name.startswith("fan")}
    assert chunks == {"fan3243_8": (1, 0), "fan3243_9": (1, 1), "fan3243_230": (28, 6),
                      "fan3443_8": (1, 0), "fan3443_9": (1, 1), "fan3443_80": (10, 0)}
    # four waves per workgroup: the last workgroup of five elements has one live wave and three shadows, of one element too
    assert all(am.COUNTS[n][1] % 4 == 1 for n in ("one_beam", "one_shell", "chain5", "strip5", "fan3243_9", "fan3443_9"))


def test_lds_of_every_configuration():
    names = [c[0] for c in w.CONFIGS]
    assert len(set(names)) == len(names)
    over = set()
    for name, env, cs, expect in w.CONFIGS:
        assert set(env) <= {"TLFEA_TANGENT_WPB"} and expect["wpb"] == int(env.get("TLFEA_TANGENT_WPB", "1"))
        for c in cs:
            m, fixed = w.mesh_of(c["mesh"])
            lds = am.assemble_rows_lds_bytes(m)
            assert (lds > 65536) == bool(expect.get("lds_over_64k")), (name, lds)
            if lds > 65536:
                over.add((c["mesh"], lds))
    assert over == {("fan3243_230", 66528), ("fan3443_80", 69408)}
    assert w.mesh_of("plate3443")[0][4].shape[0] == 192 and am.hub_row_blocks(w.mesh_of("plate3443")[0]) == 36


# ---- the judge can fail ----------------------------------------------------------------------------------------------------
class Ref:
    """oracle H of one case (undamped SVK: H = M / h + h K + h^2 rho on the pinned diagonal) with its element tangents"""

    def __init__(self, mesh, rho=w.RHO, **opt):
        self.inp = w.case_inputs(w.case(mesh, "svk", **opt))
        o = w.make_oracle(self.inp)
        o.x, o.y, o.z = (a.copy() for a in self.inp["xs"])
        self.ro, self.ci, self.val = o.assemble_hessian(w.H_STEP, rho)
        self.Ke, _ = o.element_tangents()
        self.o, self.rho = o, rho
        self.hub, self.last = self.inp["hub"], self.inp["last"]

    def block_slots(self, i, j):
        """indices into the CSR values of the 3 x 3 block (coefficient row i, coefficient column j): [3, 3]"""
        out = np.zeros((3, 3), dtype=np.int64)
        for d in range(3):
            row = self.ci[self.ro[3 * i + d]:self.ro[3 * i + d + 1]]
            k = int(np.searchsorted(row, 3 * j))
            assert row[k] == 3 * j
            out[d] = self.ro[3 * i + d] + k + np.arange(3)
        return out

    def scatter(self, val, K, e, factor, rows=None):
        """val += factor K at the rows and columns of element e's coefficients (rows: only those coefficient rows)"""
        cc = self.o.conn[e]
        for a, i in enumerate(cc):
            if rows is not None and i not in rows:
                continue
            for b, j in enumerate(cc):
                val[self.block_slots(int(i), int(j))] += factor * K[3 * a:3 * a + 3, 3 * b:3 * b + 3]

    def judged(self, val):
        return w.judge_hessian(self.ro, self.ci, val, self.ro, self.ci, self.val, val, self.hub, self.last, "judge")


@pytest.fixture(scope="module")
def beam_fan():
    return Ref("fan3243_9", hub_pinned=True)


@pytest.fixture(scope="module")
def shell_fan():
    return Ref("fan3443_9", hub_pinned=True)


def test_judge_accepts_the_oracle_and_the_tangents_add_up(beam_fan, shell_fan):
    for r in (beam_fan, shell_fan):
        assert r.judged(r.val.copy()) == (0.0, 0.0, 0.0)
        val = np.zeros_like(r.val)                                # M / h + h sum K_e + h^2 rho: the layout scatter() assumes
        o = r.o
        for i in range(o.N):
            for k in range(o.m_off[i], o.m_off[i + 1]):
                val[np.diag(r.block_slots(i, int(o.m_col[k])))] += o.m_val[k] / w.H_STEP
        for e in range(o.E):
            r.scatter(val, r.Ke[e], e, w.H_STEP)
        for i in r.inp["fixed"]:
            val[np.diag(r.block_slots(int(i), int(i)))] += w.H_STEP * w.H_STEP * r.rho
        assert w.relerr(val, r.val) < 1e-14


def test_judge_rejects_a_missing_element_block_in_the_hub_row(beam_fan):
    r = beam_fan
    val = r.val.copy()
    r.scatter(val, r.Ke[4], 4, -w.H_STEP, rows=set(am.node_coefficients(r.hub).tolist()))
    assert w.relerr(val, r.val) > 1e-6
    with pytest.raises(AssertionError):
        r.judged(val)


def test_row_view_catches_what_a_large_penalty_hides():
    """the same defect with a penalty of 1e24 on the pinned tip: against the largest entry of H it is 1e-13 and passes, against
    the largest entry of the hub's own rows it does not"""
    r = Ref("fan3243_9", rho=1e24)
    assert r.hub not in r.inp["fixed"] // 4
    val = r.val.copy()
    r.scatter(val, r.Ke[4], 4, -w.H_STEP, rows=set(am.node_coefficients(r.hub).tolist()))
    assert w.relerr(val, r.val) < w.TOL_ELEM                                       # the whole-matrix view is blind to it
    k = w.node_row_slots(r.ro, r.hub)
    assert w.relerr(val[k], r.val[k]) > 1e-3
    with pytest.raises(AssertionError, match="hub rows"):
        r.judged(val)


@pytest.mark.parametrize("fan", ["beam_fan", "shell_fan"])
def test_judge_rejects_a_shadow_wave_that_stored(fan, request):
    """the last element's blocks replaced by a second copy of element E - 2's"""
    r = request.getfixturevalue(fan)
    E = r.o.E
    val = r.val.copy()
    r.scatter(val, r.Ke[E - 1], E - 1, -w.H_STEP)
    r.scatter(val, r.Ke[E - 2], E - 1, w.H_STEP)
    k = w.node_row_slots(r.ro, r.last)
    assert w.relerr(val[k], r.val[k]) > 1e-6
    with pytest.raises(AssertionError):
        r.judged(val)


def test_judge_rejects_a_transposed_block_in_a_shell_row(shell_fan):
    r = shell_fan
    cc = r.o.conn[3]
    i, j = int(cc[5]), int(cc[10])                                # two coefficients of different nodes of shell 3
    k = r.block_slots(i, j)
    assert w.relerr(r.val[k].T, r.val[k]) > 1e-6                  # the block is not symmetric
    val = r.val.copy()
    val[k] = r.val[k].T
    with pytest.raises(AssertionError):
        r.judged(val)


def test_judge_rejects_a_missing_penalty_on_the_hub(beam_fan, shell_fan):
    for r in (beam_fan, shell_fan):
        assert set(am.node_coefficients(r.hub).tolist()) <= set(r.inp["fixed"].tolist())
        val = r.val.copy()
        for i in am.node_coefficients(r.hub):
            val[np.diag(r.block_slots(int(i), int(i)))] -= w.H_STEP * w.H_STEP * r.rho
        with pytest.raises(AssertionError):
            r.judged(val)


def test_judge_rejects_a_second_assembly_that_differs(beam_fan):
    r = beam_fan
    again = r.val.copy()
    again[7] = np.nextafter(again[7], np.inf)
    with pytest.raises(AssertionError, match="second assembly"):
        w.judge_hessian(r.ro, r.ci, r.val, r.ro, r.ci, r.val, again, r.hub, r.last, "judge")
