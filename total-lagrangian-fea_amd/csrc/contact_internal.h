// contact_internal.h -- launch wrappers of the hydroelastic contact kernels (contact_kernels.hip), called by the
// contact C-ABI (contact_api.hip).  gfx950 (MI355X) only; nothing here is part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tlfea_c.h"

namespace tlfea {

// uniform grid of the broadphase, computed on the device from the element boxes of the step
struct ContactGrid {
  double lo[3];
  double inv_cell;
  int dim[3];
  int n_cells;
};

// mesh data of a contact context (device pointers)
struct ContactMesh {
  int N, E, npe;        // nodes, elements, nodes per element (10 or 4; the first 4 are the corners)
  const int* conn;      // [npe][E] column-major
  const double* press;  // [N] nodal pressure
  const int* mesh;      // [E] mesh id per element
  int self_collision;
};

// positions: x, y, z arrays of N nodes
struct ContactPos {
  const double *x, *y, *z;
};

// element boxes [E][6] (lo xyz, hi xyz) and the grid that holds them (ContactGrid on the device, at most cell_cap cells)
void launch_contact_boxes(hipStream_t s, const ContactMesh& m, ContactPos p, double* box);
void launch_contact_grid(hipStream_t s, int E, const double* box, int cell_cap, ContactGrid* grid);
void launch_contact_cell_count(hipStream_t s, int E, const double* box, const ContactGrid* grid, int* elem_cell,
                               int* cell_cnt);
// exclusive scan of n counts by one workgroup: off[0..n], off[n] = total
void launch_contact_scan(hipStream_t s, const int* cnt, int n, int* off);
void launch_contact_cell_fill(hipStream_t s, int E, const int* elem_cell, const int* cell_off, int* cell_cur,
                              int* cell_items);
// fill == false: row_cnt[i] = candidate pairs (i, j > i) of element i; fill == true: writes them at row_off[i],
// ascending j
void launch_contact_pairs(hipStream_t s, const ContactMesh& m, const double* box, const ContactGrid* grid,
                          const int* elem_cell, const int* cell_off, const int* cell_items, bool fill, int* row_cnt,
                          const int* row_off, int2* pairs);
void launch_contact_narrowphase(hipStream_t s, const ContactMesh& m, ContactPos p, int n_pairs, const int2* pairs,
                                tlfea_contact_patch* patches, int* n_valid);
// per patch: the 8 corner contributions (tet A's corners, then tet B's) and their nodes (-1: none); node_cnt[n] += uses
void launch_contact_forces(hipStream_t s, const ContactMesh& m, ContactPos p, int n_pairs,
                           const tlfea_contact_patch* patches, const double* vel, double damping, double friction,
                           double* contrib, int* slot_node, int* node_cnt);
void launch_contact_node_fill(hipStream_t s, int n_slots, const int* slot_node, const int* node_off, int* node_cur,
                              int* node_items);
// force[3n + c] = sum of node n's contributions in ascending (patch, slot) order
void launch_contact_node_sum(hipStream_t s, int N, const int* node_off, int* node_items, const double* contrib,
                             double* force);
void launch_contact_add(hipStream_t s, int n, const double* a, const double* b, double* out);

}  // namespace tlfea
