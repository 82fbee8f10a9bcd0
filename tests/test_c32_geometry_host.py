"""Launch geometry of the single-precision polynomial step (csrc/c32_geometry.h) through a small native shim: the pure
host function that turns (rows, blocks, resident workgroups of the candidate instantiations, switches) into lanes per
row, threads per workgroup, blocks per lane issued up front, rows per group and grid.

Resident workgroups are passed in as plain numbers.  On the 256-CU device the 256-thread instantiations hold, by the
compiler's register counts for the fp16 instantiations: two-row 5 per CU at 8 and 16 lanes (96 VGPRs) and 4 at 32 (98);
one-round with the rule's lanes 8 per CU at 8 and 16 lanes (64 VGPRs) and 7 at 32 (66); one-round with half the lanes and
four blocks per lane 7 per CU (16 lanes 71 VGPRs, 8 lanes 69).

The automatic choice takes the half-lane form only from 32 lanes (the third level of the cycle, where it was measured);
from 16 lanes only TLFEA_C32_REGIME=4 selects it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAST, BANDWIDTH, LATENCY, ONE_ROUND = 0, 1, 2, 3
CUS, SLOTS = 256, 512
RES8 = (5 * CUS, 8 * CUS, 0)            # rule gives 8 lanes: no half-lane candidate
RES16 = (5 * CUS, 8 * CUS, 7 * CUS)     # rule gives 16 lanes: half = 8 lanes x 4 blocks
RES32 = (4 * CUS, 7 * CUS, 7 * CUS)     # rule gives 32 lanes: half = 16 lanes x 4 blocks


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("c32") / "libc32_geometry_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "c32_geometry_shim.cc")])
    lib = C.CDLL(str(so))
    lib.c32_shim_rule_lanes.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_int]
    return lib


def geometry(shim, N, blocks, resident, last=False, bw_rows=100000, forced_lanes=0, regime=-1, boundary=False, forced_lp=0):
    lanes = shim.c32_shim_rule_lanes(N, blocks, forced_lp, forced_lanes)
    res = (C.c_int * 3)(*resident)
    sw = (C.c_int * 5)(bw_rows, forced_lanes, regime, int(boundary), SLOTS)
    out = (C.c_int * 7)()
    shim.c32_shim_geometry(N, lanes, int(last), res, sw, out)
    g = dict(zip(("regime", "lanes", "threads", "upfront", "rows_per_group", "grid", "resident"), list(out)))
    g["rule_lanes"] = lanes
    check_invariants(g, N, resident)
    return g


def check_invariants(g, N, resident):
    assert g["lanes"] in (4, 8, 16, 32) and g["threads"] in (256, 1024) and g["grid"] >= 1
    groups = g["grid"] * (g["threads"] // g["lanes"])
    if g["regime"] == ONE_ROUND:
        half = g["lanes"] != g["rule_lanes"]
        assert g["threads"] == 256 and g["rows_per_group"] == 1 and g["upfront"] == (4 if half else 2)
        assert groups * g["rows_per_group"] >= N                                    # every row has a group: no group loops
        assert groups - N < g["threads"] // g["lanes"]                              # and no idle workgroup
        assert g["resident"] == resident[2 if half else 1]                          # the query's answer is reported ...
        assert g["grid"] * g["threads"] <= g["resident"] * 256                      # ... and all groups are resident at once
    elif g["regime"] == BANDWIDTH:
        assert g["threads"] == 256 and g["rows_per_group"] == 2 and g["upfront"] == 2 and g["grid"] <= max(1, resident[0])
    else:
        assert g["threads"] == 1024 and g["rows_per_group"] == 1 and g["upfront"] == 2 and g["grid"] <= SLOTS


def test_config_c_levels(shim):
    fine = geometry(shim, 1335961, 37716841, RES16)
    assert (fine["regime"], fine["lanes"], fine["grid"]) == (BANDWIDTH, 16, 1280)
    vertex = geometry(shim, 172081, 172081 * 14, RES8)
    assert (vertex["regime"], vertex["lanes"], vertex["rows_per_group"], vertex["grid"]) == (BANDWIDTH, 8, 2, 1280)
    third = geometry(shim, 20736, 1000000, RES32)                # 48.2 blocks per row: the rule gives 32 lanes
    assert third["rule_lanes"] == 32                             # 20 736 x 32 = 663 k threads do not fit 524 k ...
    assert (third["regime"], third["lanes"], third["upfront"], third["grid"]) == (ONE_ROUND, 16, 4, 1296)   # ... 332 k do


def test_final_step_is_always_slot_capped(shim):
    for N, blocks, res in ((1335961, 37716841, RES16), (172081, 172081 * 14, RES8), (20736, 1000000, RES32), (100, 3000, RES16)):
        for regime in (-1, 1, 2, 3, 4):
            g = geometry(shim, N, blocks, res, last=True, regime=regime)
            assert g["regime"] == LAST and g["threads"] == 1024 and g["lanes"] == g["rule_lanes"]
            assert g["grid"] == min(SLOTS, -(-N // (1024 // g["lanes"])))


def test_fits_and_does_not_fit(shim):
    # 16 lanes, 16 rows per workgroup, 2048 workgroups resident: 32 768 rows fit with full lanes, one more row does not
    assert geometry(shim, 32768, 32768 * 30, RES16) == dict(regime=ONE_ROUND, lanes=16, threads=256, upfront=2, rows_per_group=1,
                                                           grid=2048, resident=2048, rule_lanes=16)
    g = geometry(shim, 32769, 32769 * 30, RES16)                # 16 lanes do not halve by themselves: latency as before
    assert (g["regime"], g["lanes"], g["threads"], g["grid"]) == (LATENCY, 16, 1024, SLOTS)
    g = geometry(shim, 32769, 32769 * 30, RES16, regime=4)      # forced: 8 lanes x 4 blocks, 32 rows per workgroup, 1792 resident
    assert (g["regime"], g["lanes"], g["upfront"], g["grid"]) == (ONE_ROUND, 8, 4, 1025)
    assert geometry(shim, 1792 * 32, 1792 * 32 * 30, RES16, regime=4)["grid"] == 1792
    assert geometry(shim, 1792 * 32 + 1, (1792 * 32 + 1) * 30, RES16, regime=4)["regime"] == LATENCY
    # 32 lanes by the rule, 8 rows per workgroup, 1792 resident: full lanes up to 14 336 rows, then 16 lanes x 4 blocks (16
    # rows per workgroup) up to 28 672 rows, then the latency regime as before
    assert geometry(shim, 14336, 14336 * 50, RES32) == dict(regime=ONE_ROUND, lanes=32, threads=256, upfront=2, rows_per_group=1,
                                                           grid=1792, resident=1792, rule_lanes=32)
    g = geometry(shim, 14337, 14337 * 50, RES32)
    assert (g["regime"], g["lanes"], g["upfront"], g["grid"]) == (ONE_ROUND, 16, 4, 897)
    assert geometry(shim, 28672, 28672 * 50, RES32)["grid"] == 1792
    g = geometry(shim, 28673, 28673 * 50, RES32)
    assert (g["regime"], g["lanes"], g["threads"], g["grid"]) == (LATENCY, 32, 1024, SLOTS)
    # 8 lanes by the rule: no half-lane candidate
    assert geometry(shim, 65536, 65536 * 14, RES8)["regime"] == ONE_ROUND
    assert geometry(shim, 65537, 65537 * 14, RES8)["regime"] == LATENCY
    # the occupancy query answers less (or failed: 0): fall back
    assert geometry(shim, 20736, 1000000, (1024, 100, 100))["regime"] == LATENCY
    assert geometry(shim, 20736, 1000000, (1024, 0, 0))["regime"] == LATENCY
    assert geometry(shim, 20736, 1000000, (1024, 0, 1296))["regime"] == ONE_ROUND
    assert geometry(shim, 20736, 1000000, (1024, 0, 1295))["regime"] == LATENCY
    # more rows than the bandwidth threshold: two rows per group whatever fits
    assert geometry(shim, 100001, 100001 * 14, (1280, 10 ** 6, 10 ** 6))["regime"] == BANDWIDTH
    assert geometry(shim, 100000, 100000 * 14, (1280, 10 ** 6, 10 ** 6))["regime"] == ONE_ROUND


def test_switches(shim):
    # TLFEA_C32_LANES forces the lane count in every regime, and rules out the half-lane form
    for lanes in (8, 16, 32):
        for kw in (dict(), dict(last=True), dict(bw_rows=0), dict(regime=2), dict(regime=3)):
            assert geometry(shim, 5000, 5000 * 30, (1280, 2048, 2048), forced_lanes=lanes, **kw)["lanes"] == lanes
    g = geometry(shim, 20736, 1000000, RES32, forced_lanes=32)
    assert (g["regime"], g["lanes"]) == (LATENCY, 32)
    assert geometry(shim, 20736, 1000000, RES32, forced_lanes=32, regime=4)["regime"] == LATENCY
    # TLFEA_C32_BW_N=0: the 256-thread two-row geometry on every level
    for N, blocks, res in ((24, 300, RES16), (5000, 5000 * 30, RES16), (20736, 1000000, RES32)):
        g = geometry(shim, N, blocks, res, bw_rows=0)
        assert (g["regime"], g["threads"], g["rows_per_group"]) == (BANDWIDTH, 256, 2)
        assert g["grid"] == min(res[0], -(-N // (2 * (256 // g["lanes"]))))
    # forced regimes; a forced one-round that does not fit falls back to the automatic choice
    assert geometry(shim, 5000, 5000 * 30, RES16, regime=1)["regime"] == BANDWIDTH
    assert geometry(shim, 5000, 5000 * 30, RES16, regime=2)["regime"] == LATENCY
    assert geometry(shim, 5000, 5000 * 30, RES16, regime=3) == geometry(shim, 5000, 5000 * 30, RES16)
    g = geometry(shim, 5000, 5000 * 30, RES16, regime=4)
    assert (g["regime"], g["lanes"], g["upfront"], g["grid"]) == (ONE_ROUND, 8, 4, 157)
    assert geometry(shim, 5000, 5000 * 14, RES8, regime=4)["regime"] == ONE_ROUND       # 8 lanes: no half, automatic choice
    assert geometry(shim, 5000, 5000 * 14, RES8, regime=4)["lanes"] == 8
    assert geometry(shim, 1335961, 37716841, RES16, regime=3)["regime"] == BANDWIDTH
    # the multi-GPU boundary epilogue is not in the half-lane kernel: full lanes or not at all
    assert geometry(shim, 5000, 5000 * 30, RES16, boundary=True) == geometry(shim, 5000, 5000 * 30, RES16)
    assert geometry(shim, 5000, 5000 * 30, RES16, boundary=True, regime=4) == geometry(shim, 5000, 5000 * 30, RES16)
    assert geometry(shim, 20736, 1000000, RES32, boundary=True)["regime"] == LATENCY


def test_small_levels(shim):
    # smaller than one workgroup: one workgroup in every regime, the rule's lanes
    for N in (1, 3, 15):
        g = geometry(shim, N, N * 30, RES16)
        assert (g["regime"], g["lanes"], g["upfront"], g["grid"]) == (ONE_ROUND, 16, 2, 1)
        assert geometry(shim, N, N * 30, RES16, regime=2)["grid"] == 1
        assert geometry(shim, N, N * 30, RES16, bw_rows=0)["grid"] == 1
        assert geometry(shim, N, N * 30, RES16, last=True)["grid"] == 1
    assert geometry(shim, 0, 0, RES16)["regime"] == LATENCY and geometry(shim, 0, 0, RES16)["grid"] == 1
    # a masked tail group: 100 rows, 16 per workgroup
    assert geometry(shim, 100, 3000, RES16)["grid"] == 7


def test_lane_rule(shim):
    rule = lambda N, b, lp=0, f=0: shim.c32_shim_rule_lanes(N, b, lp, f)
    assert rule(1000, 18000) == 8 and rule(1000, 18001) == 16 and rule(1000, 48000) == 16 and rule(1000, 48001) == 32
    assert rule(1000, 60000, 16) == 16 and rule(1000, 10000, 32) == 32 and rule(1000, 10000, 16) == 8
    assert rule(1000, 60000, 0, 8) == 8 and rule(1000, 10000, 16, 32) == 32 and rule(1000, 60000, 0, 7) == 32


def test_gpu_configurations_meet_every_precondition_in_every_regime():
    """the table of tests/test_gpu_c32_geometry.py: the configurations of each forced regime demand, between them, a long
    row, a short row, a masked tail group and a level smaller than a workgroup on a level that runs that regime (for the
    half-lane form: on a level that runs four blocks per lane)"""
    from tests.test_gpu_c32_geometry import CONFIGS
    for regime in "1234":
        met = set()
        for name, _, _, _, pin, need in CONFIGS:
            if name[0] != regime:
                continue
            for what, level in need.items():
                assert level in pin and pin[level][0] == (ONE_ROUND if regime in "34" else int(regime))
                if regime != "4" or pin[level][2] == 4:
                    met.add(what)
        assert met == {"long", "short", "tail", "small"}, (regime, met)


def test_deterministic(shim):
    rng = np.random.default_rng(0)
    for _ in range(200):
        N = int(rng.integers(1, 300000))
        blocks = N * int(rng.integers(4, 120))
        args = dict(bw_rows=int(rng.choice([0, 100000])), regime=int(rng.choice([-1, 1, 2, 3, 4])), last=bool(rng.integers(0, 2)))
        res = (int(rng.integers(0, 1500)), int(rng.integers(0, 2500)), int(rng.integers(0, 2500)))
        assert geometry(shim, N, blocks, res, **args) == geometry(shim, N, blocks, res, **args)
