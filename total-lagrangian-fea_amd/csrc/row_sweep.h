// row_sweep.h -- which rows a lane group of the two streaming kernels (fp64 SpMV, single-precision polynomial step) walks.
//
// Shared by the kernels (solver_kernels.hip), the launchers' report of the form that ran (spmv_form, the test hook
// tlfea_newton_cg_trace) and the CPU test (tests/test_cg_np.py through tests/native/row_sweep_shim.cc): one expression
// decides whether the XCD eighths are taken, and one function turns (rows, groups per workgroup, group, grid, workgroup)
// into first row, end and stride.  No HIP, no environment, no state.
//
// XCD-aware sweep: workgroups are dealt round-robin over the 8 XCDs, so the workgroups b with the same b & 7 share one L2.
// They take ONE contiguous eighth of the rows and sweep it in tiles together, so that each XCD's gathers stay inside its
// own eighth of the vector (plus the neighbouring planes).  mode: TLFEA_XCD_ROWS, 0 never | 1 between 64 k and 600 k rows
// (where it was measured to pay) | 2 on every size from 64 k rows; always only on a grid that is a multiple of 8.
#pragma once

#if !defined(TLFEA_HD)
#if defined(__HIPCC__)
#define TLFEA_HD __host__ __device__ __forceinline__
#else
#define TLFEA_HD inline
#endif
#endif

namespace tlfea {

struct RowSweep {  // rows of this lane group: i = first, first + stride, ... < end
  int first, end, stride;
};

TLFEA_HD bool xcd_sweep_taken(int N, int grid, int mode) {
  return mode && (grid & 7) == 0 && N >= 65536 && (mode == 2 || N <= 600000);
}

// rows of one XCD's eighth: an eighth of N, rounded up to whole tiles of G rows
TLFEA_HD int xcd_eighth_rows(int N, int G) { return (((N + 7) >> 3) + G - 1) / G * G; }

// G lane groups per workgroup, group `grp` of workgroup `block` in a grid of `grid` workgroups
TLFEA_HD RowSweep row_sweep_of(int N, int G, int grp, int mode, int grid, int block) {
  RowSweep r;
  if (xcd_sweep_taken(N, grid, mode)) {
    const int nb = grid >> 3, lb = block >> 3, x = block & 7;
    const int per = xcd_eighth_rows(N, G);
    const int r0 = x * per;
    r.end = N < r0 + per ? N : r0 + per;
    r.first = r0 + lb * G + grp;
    r.stride = nb * G;
  } else {
    r.first = block * G + grp;
    r.end = N;
    r.stride = grid * G;
  }
  return r;
}

}  // namespace tlfea
