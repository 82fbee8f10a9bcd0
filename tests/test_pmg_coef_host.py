"""Coefficients of the preconditioner's polynomials and the layout of the V-cycle's coefficient table
(csrc/pmg_coef.h) through a small native shim, against the fp64 restatement in tests/precond_np.py.

Both sides perform the same double operations in the same order; a fused multiply-add on one side would move an entry by
an ulp per step of the recurrence, so 64 steps stay two orders below the 1e-13 relative bound used here.  Entries that
are zero by construction are compared exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import precond_np as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-13
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("pmgcoef") / "libpmg_coef_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "pmg_coef_shim.cc")])
    lib = C.CDLL(str(so))
    lib.pmg_shim_cheb_pairs.argtypes = [C.c_double, C.c_double, C.c_int, DP]
    lib.pmg_shim_fourth_kind_pairs.argtypes = [C.c_double, C.c_int, C.c_int, DP, DP]
    lib.pmg_shim_fill.argtypes = [C.POINTER(C.c_int), C.c_int, DP, DP]
    return lib


def constants(shim):
    out = (C.c_int * 5)()
    shim.pmg_shim_constants(out)
    return dict(zip(("max_ks", "max_kc", "max_k3", "cap", "max_deg"), list(out)))


def cheb_pairs(shim, hi, kappa, terms):
    out = np.full(2 * terms, np.nan)
    shim.pmg_shim_cheb_pairs(hi, kappa, terms, out.ctypes.data_as(DP))
    return out


def fourth_kind(shim, hi, terms, optimised):
    pairs, betas = np.full(2 * terms, np.nan), np.full(terms, np.nan)
    shim.pmg_shim_fourth_kind_pairs(hi, terms, int(optimised), pairs.ctypes.data_as(DP), betas.ctypes.data_as(DP))
    return pairs, betas


def offsets(shim, ks, ks2, kc, k3, levels):
    out = (C.c_int * 6)()
    shim.pmg_shim_offsets((C.c_int * 5)(ks, ks2, kc, k3, levels), out)
    return dict(zip(("cf_resid", "cf_restart", "cf_beta", "cf_coarse", "cf_level3", "size"), list(out)))


def fill(shim, ks, ks2, kc, k3, levels, kind, fine, vertex, level3=(0.0, 1.0)):
    n = offsets(shim, ks, ks2, kc, k3, levels)["size"]
    out = np.full(n + 4, np.nan)                       # four guard words: the fill writes size() doubles and no more
    iv = (C.c_double * 6)(*fine, *vertex, *level3)
    shim.pmg_shim_fill((C.c_int * 5)(ks, ks2, kc, k3, levels), kind, iv, out.ctypes.data_as(DP))
    assert np.all(np.isnan(out[n:])) and not np.any(np.isnan(out[:n]))
    return out[:n]


def flat(pairs):
    return np.array([v for p in pairs for v in p], dtype=np.float64)


def rel_gap(got, want):
    """largest relative difference over the non-zero entries; entries that are zero on the reference side must be zero"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    zero = want == 0.0
    assert np.array_equal(got[zero], want[zero])
    return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))) if np.any(~zero) else 0.0


@pytest.mark.parametrize("kappa", [8.0, 400.0, 6144.0])
@pytest.mark.parametrize("terms", [1, 2, 12, 24, 64])
def test_cheb_pairs_match_the_restatement(shim, terms, kappa):
    hi = 1.15 * 1.9173
    gap = rel_gap(cheb_pairs(shim, hi, kappa, terms), flat(pn.chebyshev_pairs(hi, kappa, terms)))
    print(f"cheb_pairs terms={terms} kappa={kappa}: largest relative difference {gap:.3e}")
    assert gap <= REL


@pytest.mark.parametrize("terms,optimised", [(1, True), (2, True), (3, True), (4, True), (3, False), (6, False)])
def test_fourth_kind_pairs_match_the_restatement(shim, terms, optimised):
    hi = 1.15 * 2.046
    pairs, betas = fourth_kind(shim, hi, terms, optimised)
    want_pairs, want_betas = pn.fourth_kind_pairs(hi, terms, optimised)
    assert np.array_equal(betas, np.array(want_betas))
    if optimised:
        assert np.array_equal(betas, np.array(pn.LOTTES_BETA[terms]))
    gap = rel_gap(pairs, flat(want_pairs))
    print(f"fourth_kind_pairs terms={terms} optimised={optimised}: largest relative difference {gap:.3e}")
    assert gap <= REL
    assert pairs[1] == betas[0]


@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("ks2", [2, 6, 12])
def test_table_layout_and_contents_match_cycle_state(shim, ks2, levels):
    fine, vertex, level3 = (2.2, 24.0), (2.05, 90.0), (1.9, 600.0)
    kc, k3 = 9, 11
    for ks in range(1, 13):
        fine_pairs = pn.chebyshev_pairs(*fine, ks)
        if levels == 2:
            shape = (ks, 0, kc, 0, 2)
            st = pn.cycle_state(fine_pairs, pn.chebyshev_pairs(*vertex, kc))
        else:
            shape = (ks, ks2, 0, k3, 3)
            st = pn.cycle_state(fine_pairs, pn.chebyshev_pairs(*vertex, ks2), pn.chebyshev_pairs(*level3, k3))
        off = offsets(shim, *shape)
        for name in ("cf_resid", "cf_restart", "cf_beta", "cf_coarse", "cf_level3"):
            assert off[name] == st[name], (name, ks, ks2, levels)
        assert off["size"] == len(st["coef"])
        got = fill(shim, *shape, 1, fine, vertex, level3)
        assert rel_gap(got, st["coef"]) <= REL
        # first kind: the restart pair is (0, 1/theta), every weight is 1
        theta = 0.5 * (fine[0] + fine[0] / fine[1])
        assert got[off["cf_restart"]] == 0.0 and abs(got[off["cf_restart"] + 1] * theta - 1.0) <= REL
        assert got[off["cf_restart"] + 1] == got[0]
        assert np.array_equal(got[off["cf_beta"]:off["cf_coarse"]], np.ones(12))


@pytest.mark.parametrize("kind,ks", [(4, 1), (4, 2), (4, 3), (4, 4), (3, 3), (3, 6), (4, 6)])
def test_fourth_kind_table(shim, kind, ks):
    fine, vertex = (2.2, 24.0), (2.05, 150.0)
    kc = 10
    optimised = kind == 4 and ks <= 4                   # the optimised weights are tabulated up to four terms
    pairs, betas = pn.fourth_kind_pairs(fine[0], ks, optimised)
    st = pn.cycle_state(pairs, pn.chebyshev_pairs(*vertex, kc), betas=betas)
    off = offsets(shim, ks, 0, kc, 0, 2)
    got = fill(shim, ks, 0, kc, 0, 2, kind, fine, vertex)
    assert rel_gap(got, st["coef"]) <= REL
    assert got[1] == betas[0]                                                   # z^0 = beta_1 d0
    assert got[off["cf_restart"]] == 0.0
    assert abs(got[off["cf_restart"] + 1] * (3.0 * fine[0]) / 4.0 - 1.0) <= REL  # d0' = 4/(3 hi) (SDS)^-1 res^
    assert np.array_equal(got[off["cf_beta"]:off["cf_beta"] + ks], np.array(betas))
    assert np.array_equal(got[off["cf_beta"] + ks:off["cf_coarse"]], np.ones(12 - ks))


def test_largest_tables_fit_the_allocation(shim):
    k = constants(shim)
    assert (k["max_ks"], k["max_kc"], k["max_k3"], k["max_deg"]) == (12, 64, 60, 64)
    assert offsets(shim, k["max_ks"], 0, k["max_kc"], 0, 2)["size"] <= k["cap"]
    assert offsets(shim, k["max_ks"], k["max_ks"], 0, k["max_k3"], 3)["size"] <= k["cap"]
    assert 2 * k["max_deg"] <= k["cap"]                 # the fine polynomial's pairs go through the same staging area


def test_poly_degree_rule(shim):
    deg = shim.pmg_shim_poly_degree
    assert deg(2197, 0, 64) == 12 and deg(172081, 0, 64) == 32      # the two sizes the rule was fitted on
    assert deg(10, 0, 64) == 8 and deg(2, 0, 64) == 8 and deg(0, 0, 64) == 8
    assert deg(2 ** 30, 0, 64) == 64 and deg(2 ** 30, 0, 60) == 60
    assert deg(2197, 20, 64) == 20 and deg(2197, 99, 60) == 60 and deg(2197, 1, 64) == 12
