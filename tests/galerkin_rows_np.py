"""NumPy helpers shared by tests/test_galerkin_rows_host.py and tests/test_gpu_galerkin_rows.py: the 3x3 blocks of a matrix in
the DOF-level layout [node row][d][k][e], and how far its off-diagonal blocks are from the transposes of their mirrors."""
import numpy as np


def blocks(off, vals):
    """[nnz, 3, 3]: block k of node row i holds vals[9 off[i] + d 3 deg(i) + 3 k + e]"""
    off = np.asarray(off, dtype=np.int64)
    deg = np.diff(off)
    row = np.repeat(np.arange(len(deg)), deg)
    k = np.arange(off[-1]) - off[row]
    d, e = np.arange(3)[None, :, None], np.arange(3)[None, None, :]
    return np.asarray(vals)[(9 * off[row] + 3 * k)[:, None, None] + d * (3 * deg[row])[:, None, None] + e]


def off_diagonal_asymmetry(off, cols, vals):
    """max |B(I, J) - B(J, I)^T| over the blocks with J != I (columns ascending within a row; the pattern is symmetric)"""
    off = np.asarray(off, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    B = blocks(off, vals)
    row = np.repeat(np.arange(len(off) - 1), np.diff(off))
    key = row * (len(off) - 1) + cols                                    # ascending: rows ascend, columns within them
    mirror = np.searchsorted(key, cols * (len(off) - 1) + row)
    assert np.array_equal(key[mirror], cols * (len(off) - 1) + row)
    od = row != cols
    return float(np.abs(B[od] - np.transpose(B[mirror[od]], (0, 2, 1))).max()) if od.any() else 0.0
