"""The CG trace checker (tests/cg_np.py) on the CPU: it passes the trace of a plain numpy PCG on an SPD block matrix and
fails, naming the kernel, on each fault a subtly wrong kernel of the iteration would commit; and the XCD-eighth row sweep
of csrc/row_sweep.h, through a small native shim, walks every row exactly once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import cg_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4


def spd_block_matrix(N=301, seed=2):
    """SPD matrix of 3 x 3 blocks, every stored block dense, whose node rows have 3 deg below 32, between 32 and 64 and above
    64 (the three row classes of a 32-lane product kernel): a band of half-width 3, 8 or 14 blocks, in stretches of 40 rows"""
    rng = np.random.default_rng(seed)
    half = np.array([3, 8, 14])[(np.arange(N) // 40) % 3]
    A = sp.lil_matrix((3 * N, 3 * N))
    for i in range(N):
        for j in range(i + 1, min(N, i + 1 + half[i])):
            if j - i <= half[j]:
                B = rng.normal(size=(3, 3))
                A[3 * i:3 * i + 3, 3 * j:3 * j + 3] = B
                A[3 * j:3 * j + 3, 3 * i:3 * i + 3] = B.T
    rowsum = np.asarray(abs(sp.csr_matrix(A)).sum(axis=1)).reshape(-1)
    for i in range(N):
        B = rng.normal(size=(3, 3))
        A[3 * i:3 * i + 3, 3 * i:3 * i + 3] = 0.1 * (B + B.T) + np.diag(rowsum[3 * i:3 * i + 3] + rng.uniform(1.0, 2.0, 3))
    return sp.csr_matrix(A)


@pytest.fixture(scope="module")
def system():
    H = spd_block_matrix()
    assert abs(H - H.T).max() == 0.0 and np.linalg.eigvalsh(H.toarray()).min() > 0.0
    assert all(c > 0 for c in cg_np.row_classes(H, 32)), cg_np.row_classes(H, 32)
    b = np.random.default_rng(4).normal(size=H.shape[0])
    return H, b


def test_a_correct_trace_passes(system):
    H, b = system
    for kw in (dict(), dict(spmv32=True, replace_every=2), dict(fused=False)):
        ratios = cg_np.check_trace(H, b, cg_np.numpy_trace(H, b, K, **kw))
        print(kw, {k: "%.3f" % v for k, v in ratios.items()})
        assert set(ratios) >= {"product", "direction", "update", "dot", "slots", "z"} and max(ratios.values()) <= 1.0


# fault -> the kernel the checker must name
CAUGHT_AS = {"q_misses_last_block": "product q = H p", "q_row_doubled": "product q = H p", "pq_slot_dropped": "p.q sum",
             "beta_slots_swapped": "direction p = z + beta p", "p_old_for_p_new": "update x += alpha p",
             "last_row_left_stale": "product q = H p", "float32_matrix_unreported": "product q = H p"}


@pytest.mark.parametrize("fault", cg_np.FAULTS)
def test_each_injected_fault_is_caught(system, fault):
    H, b = system
    assert set(CAUGHT_AS) == set(cg_np.FAULTS)
    row = 100   # a long row: its last column block is one of 29
    tr = cg_np.numpy_trace(H, b, K, fault=fault, fault_it=2, fault_row=row)
    with pytest.raises(cg_np.TraceError) as e:
        cg_np.check_trace(H, b, tr)
    msg = str(e.value)
    print(fault, "->", msg)
    # the unreported float32 copy is every iteration's product, the others are committed in iteration 2 and nowhere before
    assert msg.startswith(CAUGHT_AS[fault] + ", iteration %d" % (0 if fault == "float32_matrix_unreported" else 2)), msg
    if fault in ("q_misses_last_block", "q_row_doubled"):
        assert "(node row %d)" % row in msg, msg
    if fault == "last_row_left_stale":
        assert "(node row %d)" % (H.shape[0] // 3 - 1) in msg, msg


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("rowsweep") / "librow_sweep_shim.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "native", "row_sweep_shim.cc")])
    lib = C.CDLL(str(so))
    lib.row_sweep_shim_cover.restype = C.c_longlong
    lib.row_sweep_shim_cover.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return lib


def test_xcd_predicate(shim):
    taken = lambda N, grid, mode=1: bool(shim.row_sweep_shim_taken(N, grid, mode))
    assert not taken(65535, 512) and taken(65536, 512) and taken(600000, 512) and not taken(600001, 512)
    assert taken(600001, 512, 2) and not taken(65535, 512, 2) and not taken(100000, 512, 0)
    assert not taken(100000, 508) and not taken(100000, 511) and taken(100000, 504) and taken(100000, 8)
    # the box of tests/test_gpu_cg_trace.py: an eighth rounds to 8 224 rows at 32 lanes and to 8 256 at 16, the last is short
    N = 41 * 41 * 39
    assert cg_np.spmv_grid(N) == 512 and taken(N, 512)
    assert shim.row_sweep_shim_eighth(N, 32) == 8224 and shim.row_sweep_shim_eighth(N, 64) == 8256
    assert 0 < N - 7 * 8224 < 8224 and 0 < N - 7 * 8256 < 8256


@pytest.mark.parametrize("G", [32, 64])
def test_the_eighths_cover_every_row_exactly_once(shim, G):
    for N in (65536 + 1, 65559, 100003, 599999, 65536):
        for grid in (512, 8, 504, 64):
            for mode in (1, 2, 0):
                if N % (8 * G) == 0 and N != 65536:
                    continue
                count = np.zeros(N, dtype=np.int32)
                outside = shim.row_sweep_shim_cover(N, G, grid, mode, count.ctypes.data_as(C.POINTER(C.c_int)))
                assert outside == 0 and count.min() == 1 and count.max() == 1, (N, G, grid, mode, outside, count.min(), count.max())
    assert all(N % (8 * G) != 0 for N in (65537, 65559, 100003, 599999))
    # a grid that is no multiple of 8 and sizes outside the window fall back to the plain tiled sweep, which covers too
    for N, grid in ((70000, 500), (1000, 32), (700001, 512)):
        count = np.zeros(N, dtype=np.int32)
        assert shim.row_sweep_shim_cover(N, G, grid, 1, count.ctypes.data_as(C.POINTER(C.c_int))) == 0
        assert count.min() == 1 and count.max() == 1
