"""The element stage of the ANCF-3243 beam and the ANCF-3443 shell -- host mass values and ds/du, residual_kernel<8,12> /
<16,48>, grad_kernel, tangent_blocks_kernel<8,12,6> / <16,48,6>, assemble_rows_kernel<8> / <16> (csrc/elem_kernels.hip,
csrc/data_api.hip) -- in every launch form, on the meshes of tests/ancf_edge_meshes.py: one element, five elements (with
TLFEA_TANGENT_WPB=4 one live wave and three shadows in the last workgroup), hubs whose row of H fills whole 8-element chunks
or one element more, hub rows above 64 KiB of LDS, per-element dimensions, nodes of no element.  Each configuration of
tests/ancf_forms_worker.py runs in a child process (the library reads its switches once), one child at a time; the worker
asserts the launch form through tlfea_newton_get_assembly_form and the stage counters, this file judges every downloaded
number on the CPU against orc.AncfOracle on the same inputs -- never with the project's own kernels.

Bounds (tests/test_gpu_parity.py, as tests/test_gpu_elem_forms.py states them): index arrays bit-equal; mass and det J to
1e-13; ds/du, F, P, f_int, the gradient and H to TOL_ELEM = 1e-12 of the largest entry; the second assembly the same bits;
H symmetric to 1e-12 max|H|.  The largest entry of H can be a pinned penalty, so the rows of the hub node and the rows of
the last element's nodes are judged again, each against the largest entry of those rows alone.  The hub rows of the large
fans sum 230 and 80 element blocks: two fp64 summation orders of n terms differ by about 2 n eps of the sum of magnitudes,
5e-14 or less, inside TOL_ELEM.  Configurations that share mesh, material and state must agree with each other to TOL_ELEM
between one and four waves per workgroup (the report says whether bit for bit; that is not required).  That the judge
rejects a wrong H is shown without a GPU in tests/test_ancf_edge_meshes.py.  Figures: profiles/ancf_forms.txt, written by
running this file with TLFEA_ANCF_FORMS_REPORT=<file> (every line the tests print is then appended to that file too; the
variable is read here only, the children never see it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ancf_forms_worker as w

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in w.CONFIGS]
# what the HIP runtime and the driver say when a kernel has faulted, in an error message of a child that did not die of a signal
GPU_FAULT_SIGNS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorIllegalAddress",
                   "hipErrorLaunchFailure", "unspecified launch failure", "HW Exception", "GPU Hang", "Aborted")


class Runs:
    """children run once each, strictly one at a time; oracle references once per case"""

    def __init__(self, tmp):
        self.tmp, self.done, self.refs = tmp, {}, {}

    def worker(self, name):
        if name in self.done:
            return self.done[name]
        _, env, cases, expect = next(c for c in w.CONFIGS if c[0] == name)
        npz = str(self.tmp / (name + ".npz"))
        cfg = dict(name=name, env=env, cases=cases, expect=expect)
        clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ancf_forms_worker.py"), json.dumps(cfg), npz], cwd=ROOT,
                               env=dict(clean, **env), capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("%s: the worker hung -- nothing more is started on this GPU" % name, returncode=3)
        if r.returncode < 0 or r.returncode in (134, 139):  # killed by a signal: a GPU fault or an abort ends the session
            pytest.exit("%s: the worker died with %d -- nothing more is started on this GPU\n%s" % (name, r.returncode, r.stderr[-3000:]),
                        returncode=3)
        if r.returncode != 0 and any(sign in r.stdout + r.stderr for sign in GPU_FAULT_SIGNS):
            # a fault the runtime reported as an error instead of a signal: the card is not to be used again either
            pytest.exit("%s: the worker met a GPU fault -- nothing more is started on this GPU\n%s" % (name, r.stderr[-3000:]), returncode=3)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        self.done[name] = (out, dict(np.load(npz, allow_pickle=False)))
        return self.done[name]

    def reference(self, c):
        key = json.dumps(c, sort_keys=True)
        if key not in self.refs:
            inp = w.case_inputs(c)
            self.refs[key] = (inp, w.oracle_reference(inp))
        return self.refs[key]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("ancf_forms"))


def report(line):
    print(line)
    path = os.environ.get("TLFEA_ANCF_FORMS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def case_data(data, k):
    return {key[len("c%d_" % k):]: v for key, v in data.items() if key.startswith("c%d_" % k)}


def free_gradient_error(inp, d, ref):
    """reported, not judged: the gradient on the coefficients that are not pinned, against its largest entry there (the
    penalty term of a pinned coefficient can be the largest entry of the whole gradient)"""
    free = np.ones(inp["N"], dtype=bool)
    free[inp["fixed"]] = False
    return w.relerr(d["g"].reshape(-1, 3)[free], ref["g"].reshape(-1, 3)[free])


@pytest.mark.parametrize("name", NAMES)
def test_ancf_form(runs, name):
    out, data = runs.worker(name)
    for k, rec in enumerate(out["cases"]):
        c, form = rec["case"], rec["form"]
        inp, ref = runs.reference(c)
        d = case_data(data, k)
        who = "%s[%s %s]" % (name, c["mesh"], c["mat"])
        same = all(d[a].shape == np.shape(ref[b]) for a, b in (("detJ", "detJ"), ("dsdu", "dsdu"), ("m_val", "m_val"), ("F", "F"), ("P", "P"),
                                                                ("f_int", "f_int"), ("g", "g"), ("H_val", "val")))
        measured = {}
        if same:
            measured = {q: w.relerr(d[a], ref[b]) for q, a, b in (("detJ", "detJ", "detJ"), ("mass", "m_val", "m_val"), ("dsdu", "dsdu", "dsdu"),
                                                                  ("F", "F", "F"), ("P", "P", "P"), ("f_int", "f_int", "f_int"),
                                                                  ("g", "g", "g"), ("H", "H_val", "val"))}
            measured["g_free"] = free_gradient_error(inp, d, ref)
            for tag, nodes in (("H_hub", inp["hub"]), ("H_last", inp["last"])):
                slots = w.node_row_slots(ref["ro"], nodes)
                measured[tag] = w.relerr(d["H_val"][slots], ref["val"][slots])
        report("%-26s %-16s %-10s%s N %4d E %4d | mode %d wpb %d lds %6d wg %4d | gradient form %d | stage counts tangent %d assemble %d | "
               "second assembly bit-equal %s | relerr %s"
               % (name, c["mesh"], c["mat"], " hub pinned" if c.get("hub_pinned") else "", rec["N"], rec["E"], form["mode"], form["tangent_wpb"],
                  form["lds_bytes"], form["workgroups"], rec["gradient_form"], rec["stage_counts"]["tangent_blocks"],
                  rec["stage_counts"]["assemble_rows"], bool(np.array_equal(d["H_val"], d["H_val2"])),
                  " ".join("%s %.1e" % kv for kv in measured.items())))
        assert same, (who, "array shapes differ from the oracle's")
        w.judge_case(inp, ref, d, who)


def test_forms_agree_with_each_other(runs):
    """configurations that share mesh, material, pinned coefficients and state: their H agree to TOL_ELEM between one and
    four waves per workgroup; every WPB-4 configuration has such a partner"""
    groups = {}
    for name in NAMES:
        out, data = runs.worker(name)
        for k, rec in enumerate(out["cases"]):
            groups.setdefault(json.dumps(rec["case"], sort_keys=True), []).append((name, rec["form"], case_data(data, k)))
    compared = 0
    for key, members in groups.items():
        base = members[0]
        for name, form, d in members[1:]:
            assert {form["tangent_wpb"], base[1]["tangent_wpb"]} == {1, 4}, (key, name, base[0])
            err = {q: w.relerr(d[q], base[2][q]) for q in ("H_val", "g", "f_int")}
            report("agree %-62s %-22s (wpb %d) vs %-22s (wpb %d): H %.1e g %.1e f_int %.1e, H bit for bit %s"
                   % (key, name, form["tangent_wpb"], base[0], base[1]["tangent_wpb"], err["H_val"], err["g"], err["f_int"],
                      bool(np.array_equal(d["H_val"], base[2]["H_val"]))))
            assert max(err.values()) < w.TOL_ELEM, (key, name, base[0], err)
            compared += 1
    wpb4_cases = sum(len(c[2]) for c in w.CONFIGS if c[1])
    assert compared == wpb4_cases == 3 * len(w.WPB4_MESHES) + 2 * len(w.HUB_MESHES)
