// C entry points of csrc/row_sweep.h for tests/test_cg_np.py (the header is pure host code when no HIP compiler reads it).
#include "../../total-lagrangian-fea_amd/csrc/row_sweep.h"

extern "C" int row_sweep_shim_taken(int N, int grid, int mode) { return tlfea::xcd_sweep_taken(N, grid, mode) ? 1 : 0; }
extern "C" int row_sweep_shim_eighth(int N, int G) { return tlfea::xcd_eighth_rows(N, G); }

// count[i] += 1 for every row i that some lane group of some workgroup walks; returns the rows walked at or beyond N
extern "C" long long row_sweep_shim_cover(int N, int G, int grid, int mode, int* count) {
  long long outside = 0;
  for (int b = 0; b < grid; b++)
    for (int g = 0; g < G; g++) {
      const tlfea::RowSweep r = tlfea::row_sweep_of(N, G, g, mode, grid, b);
      for (long long i = r.first; i < r.end; i += r.stride) {
        if (i < 0 || i >= N) outside++;
        else count[i]++;
      }
    }
  return outside;
}
