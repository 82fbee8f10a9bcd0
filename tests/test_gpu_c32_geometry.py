"""Every launch regime of the single-precision polynomial step (csrc/c32_geometry.h), pinned with TLFEA_C32_REGIME and
checked as an operator: ApplyPreconditioner against the fp64 restatement tests/precond_np.py, by the rule of
tests/test_gpu_precond_operator.py -- error and symmetry defect within 8 x the CPU fp32 floor of the configuration
(computed here from numpy alone), never looser than 1e-3, floor itself at most 1e-4; M^-1 0 exactly zero; bitwise repeat;
the CG iteration count against the numpy PCG within the CPU's own float32 / float64 gap + 2.

Each configuration is one child process (tests/c32_geometry_worker.py; the library reads its switches once) under a time
limit.  The worker fails unless the geometry hook reports the pinned regime, lane count and up-front blocks on every
level named in `pin` after every application and after the solve, unless every one-round launch is within what the
occupancy query answered for its instantiation (the hook reports that too), and unless the level named in `need` shows
the precondition in the geometry that ran:
  long   a row with more blocks than lanes x up-front slots   (the further-rounds loop)
  short  a row with fewer blocks than lanes                   (masked lanes in the first slot)
  tail   rows no multiple of the rows per workgroup           (masked tail group)
  small  fewer rows than one workgroup holds
The fixtures (rows; blocks per row min..max; checked on the CPU): res2 466 fine rows 10..57 and 90 vertex rows 5..14;
bunny 2095 rows 10..170, 352 vertex rows 5..36, 54 third-level rows 16..54; plate3443 884 rows 16..36; beam_3x2x1 105
rows 10..42, 24 vertex rows 5..11, 4 third-level rows of 4 blocks.  No fixture alone has all four in every regime (no level
of res2, bunny or plate3443 is smaller than a 256-thread workgroup of 8-lane groups), so beam_3x2x1 joins them, and
tests/test_c32_geometry_host.py (CPU) asserts that the configurations of each regime demand all four between them.
For the half-lane form only the levels that ran it count: TLFEA_LP_LANES=32 raises the rule to 32 lanes on the beam so
that its 4-row third level runs 16 lanes x 4 blocks.

plate3443's CG count hangs on fp32 rounding: 163 iterations with float64 work vectors against 284 with float32 ones on the
CPU, so its allowed distance to the numpy count is 123; one run gave 269 / 274 / 274 / 278 in regimes 1 / 2 / 3 / 4.

Regimes 2 (latency, 1024-thread workgroups) and 3 (one round, the same kernel in 256-thread workgroups) must agree
bitwise: same lanes, same blocks per lane, same order of the row sums."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import precond_np as pn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AUTO = [0, 0.0, 0, 0]
L3 = {"TLFEA_PMG_LEVELS": "3"}
BANDWIDTH, LATENCY, ONE_ROUND = 1, 2, 3
# name, problem, environment, expect (precond_worker), pin {level: [regime, lanes, up-front]}, need {precondition: level}
CONFIGS = [
    ("1_bandwidth_res2", "res2", {}, dict(precond=2, levels=2), {0: [1, 16, 2], 1: [1, 8, 2]}, dict(long=0, short=0, tail=0)),
    ("1_bandwidth_bunny3", "bunny", L3, dict(precond=2, levels=3), {0: [1, 16, 2], 1: [1, 8, 2], 2: [1, 16, 2]}, dict(long=1, short=1, tail=2)),
    ("1_bandwidth_plate", "plate3443", {}, dict(precond=1, block=12), {0: [1, 16, 2]}, dict(long=0, tail=0)),
    ("1_bandwidth_beam", "beam_3x2x1", {}, dict(precond=2, levels=2), {0: [1, 16, 2], 1: [1, 8, 2]}, dict(small=1, tail=0)),
    ("2_latency_res2", "res2", {}, dict(precond=2, levels=2), {0: [2, 16, 2], 1: [2, 8, 2]}, dict(long=0, short=0, tail=0, small=1)),
    ("2_latency_bunny3", "bunny", L3, dict(precond=2, levels=3), {0: [2, 16, 2], 1: [2, 8, 2], 2: [2, 16, 2]}, dict(long=1, short=1, tail=0, small=2)),
    ("2_latency_plate", "plate3443", {}, dict(precond=1, block=12), {0: [2, 16, 2]}, dict(long=0, tail=0)),
    ("3_one_round_res2", "res2", {}, dict(precond=2, levels=2), {0: [3, 16, 2], 1: [3, 8, 2]}, dict(long=0, short=0, tail=0)),
    ("3_one_round_bunny3", "bunny", L3, dict(precond=2, levels=3), {0: [3, 16, 2], 1: [3, 8, 2], 2: [3, 16, 2]}, dict(long=1, short=1, tail=2)),
    ("3_one_round_plate", "plate3443", {}, dict(precond=1, block=12), {0: [3, 16, 2]}, dict(long=0, tail=0)),
    ("3_one_round_beam", "beam_3x2x1", {}, dict(precond=2, levels=2), {0: [3, 16, 2], 1: [3, 8, 2]}, dict(small=1, tail=0)),
    ("4_half_lanes_res2", "res2", {}, dict(precond=2, levels=2), {0: [3, 8, 4], 1: [3, 8, 2]}, dict(long=0, tail=0)),
    ("4_half_lanes_bunny3", "bunny", L3, dict(precond=2, levels=3), {0: [3, 8, 4], 1: [3, 8, 2], 2: [3, 8, 4]}, dict(long=0, tail=2)),
    ("4_half_lanes_plate", "plate3443", {}, dict(precond=1, block=12), {0: [3, 8, 4]}, dict(long=0, tail=0)),
    ("4_half_lanes_beam3", "beam_3x2x1", dict(L3, TLFEA_LP_LANES="32"), dict(precond=2, levels=3),
     {0: [3, 16, 4], 1: [3, 16, 4], 2: [3, 16, 4]}, dict(short=0, tail=0, small=2)),
]
BY_NAME = {c[0]: c for c in CONFIGS}


def run_worker(name, tmp_dir):
    _, problem, env, expect, pin, need = BY_NAME[name]
    npz = os.path.join(tmp_dir, name + ".npz")
    cfg = dict(name=name, problem=problem, opts=AUTO, expect=expect, pin=pin, need=need)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("TLFEA_") or k == "TLFEA_LIB_PATH"}
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "c32_geometry_worker.py"), json.dumps(cfg), npz]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(clean, TLFEA_C32_REGIME=name[0], **env), capture_output=True, text=True)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):   # a hang, a GPU fault or an abort ends the session
        pytest.exit("%s: the worker ended with %d -- nothing more is started on this GPU\n%s" % (name, r.returncode, r.stderr[-3000:]),
                    returncode=3)
    return r, npz


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """worker results, one child per configuration, started on first use and kept for the tests that share them"""
    tmp_dir, cache = str(tmp_path_factory.mktemp("c32")), {}

    def get(name):
        if name not in cache:
            cache[name] = run_worker(name, tmp_dir)
        return cache[name]
    return get


def state_of(data, which):
    st = {k: int(v) for k, v in zip(data["layout_keys"], data["layout" + which])}
    st["coef"] = data["coef" + which]
    return st


@pytest.mark.parametrize("name", [c[0] for c in CONFIGS])
def test_regime_is_the_restated_operator(name, runs):
    r, npz = runs(name)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    data = dict(np.load(npz, allow_pickle=False))
    names = [str(v) for v in data["names"]]
    st = state_of(data, "")
    op64, op32 = pn.operator_from(data, st, np.float64), pn.operator_from(data, st, np.float32)
    floors = {}
    for nm, r_ in zip(names, data["R"]):
        z64 = op64(r_)
        floors[nm] = float(np.linalg.norm(op32(r_) - z64) / np.linalg.norm(z64))
    floor = max(floors.values())
    bound = min(8.0 * floor, 1e-3)
    st_e = state_of(data, "_solve")
    H = pn.unpack_csr("H", data)
    it64 = pn.pcg(H, data["b"], pn.operator_from(data, st_e, np.float64), 1e-12)[1]
    it32 = pn.pcg(H, data["b"], pn.operator_from(data, st_e, np.float32), 1e-12)[1]
    gap = abs(it32 - it64) + 2
    err, sym = max(out["err"].values()), max(out["sym"])
    print("%-22s floor %.2e  bound %.2e  err %.2e [%s]  sym %.2e  its gpu %d numpy %d (cpu f32 %d f64 %d)  geometry %s"
          % (name, floor, bound, err, max(out["err"], key=out["err"].get), sym, out["its_gpu"], out["its_np"], it32, it64,
             json.dumps(out["geometry"][-1])))
    assert out["store"] != 64 and out["finite"]
    assert floor <= 1e-4, (name, floor)
    assert out["zero_exact"], "M^-1 0 is not exactly zero"
    assert all(e <= bound for e in out["err"].values()), (bound, out["err"])
    assert sym <= bound, (bound, out["sym"])
    assert all(v > 0.0 for v in out["xMx"].values()), out["xMx"]
    assert out["bitwise_repeat"] and out["bitwise_block_vs_single"]
    assert out["rel_gpu"] <= 1e-12 and out["rel_np"] <= 1e-12 and out["x_relerr"] <= 1e-8
    assert abs(out["its_gpu"] - out["its_np"]) <= gap, (out["its_gpu"], out["its_np"], it32, it64)


@pytest.mark.parametrize("fixture", ["res2", "bunny3", "plate"])
def test_one_round_with_the_rules_lanes_has_the_bits_of_the_latency_regime(fixture, runs):
    shas = []
    for name in ("2_latency_" + fixture, "3_one_round_" + fixture):
        r, _ = runs(name)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        shas.append(json.loads(r.stdout.strip().splitlines()[-1])["sha"])
    assert shas[0] is not None and shas[0] == shas[1]
