// contact_api.hip -- C-ABI of the hydroelastic contact subsystem (include/tlfea_c.h, tlfea_contact_*): buffer
// ownership and the launch sequence of one contact step (contact_kernels.hip).  The number of launches per step does
// not depend on the mesh; the one device-to-host read per step is the candidate-pair count, which sizes the pair
// buffers before they are filled (they grow, the list is never truncated).
#include "api_common.h"
#include "contact_internal.h"

using namespace tlfea;

struct tlfea_contact_s {
  int N = 0, E = 0, npe = 0, self = 0;
  hipStream_t stream = nullptr;  // the default stream, as the element object
  int *d_conn = nullptr, *d_mesh = nullptr;
  double* d_press = nullptr;
  // bound positions: an element object (read at every step) or a column-major device buffer
  tlfea_t10_t t10 = nullptr;
  const double* d_nodes = nullptr;
  // broadphase
  int cell_cap = 0;
  double* d_box = nullptr;
  ContactGrid* d_grid = nullptr;
  int *d_elem_cell = nullptr, *d_cell_cnt = nullptr, *d_cell_off = nullptr, *d_cell_cur = nullptr,
      *d_cell_items = nullptr, *d_row_cnt = nullptr, *d_row_off = nullptr;
  // pairs and everything sized by them
  int pair_cap = 0, n_pairs = 0;
  int2* d_pairs = nullptr;
  tlfea_contact_patch* d_patches = nullptr;
  double* d_contrib = nullptr;
  int *d_slot_node = nullptr, *d_node_items = nullptr;
  // nodal sum
  int *d_node_cnt = nullptr, *d_node_off = nullptr, *d_node_cur = nullptr, *d_n_valid = nullptr;
  double *d_force = nullptr, *d_base = nullptr;

  ContactMesh mesh() const { return ContactMesh{N, E, npe, d_conn, d_press, d_mesh, self}; }

  int positions(ContactPos* p) const {
    if (t10) {
      p->x = tlfea_t10_x12_device_ptr(t10);
      p->y = tlfea_t10_y12_device_ptr(t10);
      p->z = tlfea_t10_z12_device_ptr(t10);
    } else if (d_nodes) {
      p->x = d_nodes;
      p->y = d_nodes + N;
      p->z = d_nodes + 2 * (size_t)N;
    } else {
      return api_fail("tlfea_contact_step: no positions bound (tlfea_contact_bind_t10 or tlfea_contact_bind_nodes)");
    }
    return 0;
  }

  int grow_pairs(int need) {
    if (need <= pair_cap) return 0;
    const long long cap = std::max<long long>((long long)need + need / 4, 2LL * pair_cap);
    if (cap * 8 > 0x7fffffffLL) return api_fail("tlfea_contact_step: " + std::to_string(need) + " candidate pairs exceed the capacity of the contact buffers");
    dfree(d_pairs), dfree(d_patches), dfree(d_contrib), dfree(d_slot_node), dfree(d_node_items);
    pair_cap = 0;
    if (dmalloc(&d_pairs, cap) || dmalloc(&d_patches, cap) || dmalloc(&d_contrib, cap * 24) ||
        dmalloc(&d_slot_node, cap * 8) || dmalloc(&d_node_items, cap * 8))
      return 1;
    pair_cap = (int)cap;
    return 0;
  }

  void release() {
    dfree(d_conn), dfree(d_mesh), dfree(d_press), dfree(d_box), dfree(d_grid), dfree(d_elem_cell), dfree(d_cell_cnt);
    dfree(d_cell_off), dfree(d_cell_cur), dfree(d_cell_items), dfree(d_row_cnt), dfree(d_row_off), dfree(d_pairs);
    dfree(d_patches), dfree(d_contrib), dfree(d_slot_node), dfree(d_node_items), dfree(d_node_cnt), dfree(d_node_off);
    dfree(d_node_cur), dfree(d_n_valid), dfree(d_force), dfree(d_base);
  }
};

// HydroelasticPatchCollisionSystem::HydroelasticPatchCollisionSystem (HydroelasticPatchCollisionSystem.cc)
extern "C" int tlfea_contact_create(int n_nodes, int n_elems, int nodes_per_elem, const int* conn_colmajor,
                                    const double* pressure, const int* elem_mesh_ids, int self_collision,
                                    tlfea_contact_t* out) {
  if (!out) return api_fail("tlfea_contact_create: out is NULL");
  *out = nullptr;
  if (n_nodes <= 0 || n_elems <= 0 || (nodes_per_elem != 10 && nodes_per_elem != 4) || !conn_colmajor || !pressure)
    return api_fail("tlfea_contact_create: needs n_nodes > 0, n_elems > 0, 10 or 4 nodes per element, connectivity "
                    "and pressure");
  const size_t nc = (size_t)n_elems * nodes_per_elem;
  for (size_t k = 0; k < nc; k++)
    if (conn_colmajor[k] < 0 || conn_colmajor[k] >= n_nodes)
      return api_fail("tlfea_contact_create: connectivity entry " + std::to_string(k) + " = " +
                      std::to_string(conn_colmajor[k]) + " is not a node id below " + std::to_string(n_nodes));
  std::vector<int> mesh(n_elems, 0);
  if (elem_mesh_ids) mesh.assign(elem_mesh_ids, elem_mesh_ids + n_elems);
  auto* c = new tlfea_contact_s;
  c->N = n_nodes, c->E = n_elems, c->npe = nodes_per_elem, c->self = self_collision ? 1 : 0;
  c->cell_cap = std::max(1024, 2 * n_elems);
  const size_t N = n_nodes, E = n_elems;
  int rc = dmalloc(&c->d_conn, nc) || dmalloc(&c->d_mesh, E) || dmalloc(&c->d_press, N) || dmalloc(&c->d_box, 6 * E) ||
           dmalloc(&c->d_grid, 1) || dmalloc(&c->d_elem_cell, E) || dmalloc(&c->d_cell_cnt, c->cell_cap) ||
           dmalloc(&c->d_cell_off, c->cell_cap + 1) || dmalloc(&c->d_cell_cur, c->cell_cap) ||
           dmalloc(&c->d_cell_items, E) || dmalloc(&c->d_row_cnt, E) || dmalloc(&c->d_row_off, E + 1) ||
           dmalloc(&c->d_node_cnt, N) || dmalloc(&c->d_node_off, N + 1) || dmalloc(&c->d_node_cur, N) ||
           dmalloc(&c->d_n_valid, 1) || dmalloc(&c->d_force, 3 * N) || dmalloc(&c->d_base, 3 * N) ||
           c->grow_pairs(std::max(1024, 4 * n_elems));
  if (!rc) {
    hipError_t e = hipMemcpy(c->d_conn, conn_colmajor, nc * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_mesh, mesh.data(), E * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_press, pressure, N * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(c->d_force, 0, 3 * N * sizeof(double));
    if (e == hipSuccess) e = hipMemset(c->d_base, 0, 3 * N * sizeof(double));
    if (e == hipSuccess) e = hipMemset(c->d_n_valid, 0, sizeof(int));
    if (e != hipSuccess) rc = api_fail(std::string("tlfea_contact_create: ") + hipGetErrorString(e));
  }
  if (rc) {
    c->release();
    delete c;
    return rc;
  }
  *out = c;
  return 0;
}

// ~HydroelasticPatchCollisionSystem
extern "C" int tlfea_contact_destroy(tlfea_contact_t c) {
  if (!c) return api_fail("tlfea_contact_destroy: NULL context");
  (void)hipDeviceSynchronize();
  c->release();
  delete c;
  return 0;
}

// BindNodesDevicePtr, element-object form: x / y / z are separate allocations in this engine
extern "C" int tlfea_contact_bind_t10(tlfea_contact_t c, tlfea_t10_t data) {
  if (!c || !data) return api_fail("tlfea_contact_bind_t10: NULL argument");
  if (tlfea_t10_get_n_coef(data) != c->N)
    return api_fail("tlfea_contact_bind_t10: the element object has " + std::to_string(tlfea_t10_get_n_coef(data)) +
                    " nodes, the contact context " + std::to_string(c->N));
  c->t10 = data;
  c->d_nodes = nullptr;
  return 0;
}

// BindNodesDevicePtr(d_nodes): [x..., y..., z...]
extern "C" int tlfea_contact_bind_nodes(tlfea_contact_t c, const double* d_colmajor, int n_nodes) {
  if (!c || !d_colmajor) return api_fail("tlfea_contact_bind_nodes: NULL argument");
  if (n_nodes != c->N)
    return api_fail("tlfea_contact_bind_nodes: " + std::to_string(n_nodes) + " nodes, the contact context has " +
                    std::to_string(c->N));
  c->d_nodes = d_colmajor;
  c->t10 = nullptr;
  return 0;
}

// Step(CollisionSystemInput, CollisionSystemParams): HydroelasticPatchCollisionSystem.cc (broadphase, narrowphase,
// computeExternalForces)
extern "C" int tlfea_contact_step(tlfea_contact_t c, const double* d_vel, double damping, double friction) {
  if (!c) return api_fail("tlfea_contact_step: NULL context");
  ContactPos p;
  if (int rc = c->positions(&p)) return rc;
  const hipStream_t s = c->stream;
  const ContactMesh m = c->mesh();
  // broadphase: element boxes -> grid -> cell lists -> pair rows counted, scanned, filled (each row sorted: the
  // order of a cell's members, claimed with atomics, does not reach the output)
  launch_contact_boxes(s, m, p, c->d_box);
  launch_contact_grid(s, c->E, c->d_box, c->cell_cap, c->d_grid);
  HIP_TRY(hipMemsetAsync(c->d_cell_cnt, 0, c->cell_cap * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(c->d_cell_cur, 0, c->cell_cap * sizeof(int), s));
  launch_contact_cell_count(s, c->E, c->d_box, c->d_grid, c->d_elem_cell, c->d_cell_cnt);
  launch_contact_scan(s, c->d_cell_cnt, c->cell_cap, c->d_cell_off);
  launch_contact_cell_fill(s, c->E, c->d_elem_cell, c->d_cell_off, c->d_cell_cur, c->d_cell_items);
  launch_contact_pairs(s, m, c->d_box, c->d_grid, c->d_elem_cell, c->d_cell_off, c->d_cell_items, false, c->d_row_cnt,
                       nullptr, nullptr);
  launch_contact_scan(s, c->d_row_cnt, c->E, c->d_row_off);
  int total = 0;
  HIP_TRY(hipMemcpyAsync(&total, c->d_row_off + c->E, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (total < 0) return api_fail("tlfea_contact_step: candidate-pair count overflowed");
  if (int rc = c->grow_pairs(total)) return rc;
  c->n_pairs = total;
  launch_contact_pairs(s, m, c->d_box, c->d_grid, c->d_elem_cell, c->d_cell_off, c->d_cell_items, true, c->d_row_cnt,
                       c->d_row_off, c->d_pairs);
  // narrowphase: one patch per pair
  HIP_TRY(hipMemsetAsync(c->d_n_valid, 0, sizeof(int), s));
  HIP_TRY(hipMemsetAsync(c->d_node_cnt, 0, c->N * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(c->d_node_cur, 0, c->N * sizeof(int), s));
  launch_contact_narrowphase(s, m, p, total, c->d_pairs, c->d_patches, c->d_n_valid);
  // forces: 8 corner contributions per patch, node lists counted / scanned / filled, summed in patch order
  launch_contact_forces(s, m, p, total, c->d_patches, d_vel, damping, friction, c->d_contrib, c->d_slot_node,
                        c->d_node_cnt);
  launch_contact_scan(s, c->d_node_cnt, c->N, c->d_node_off);
  launch_contact_node_fill(s, 8 * total, c->d_slot_node, c->d_node_off, c->d_node_cur, c->d_node_items);
  launch_contact_node_sum(s, c->N, c->d_node_off, c->d_node_items, c->d_contrib, c->d_force);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int tlfea_contact_set_base_force(tlfea_contact_t c, const double* f, int n) {
  if (!c || !f) return api_fail("tlfea_contact_set_base_force: NULL argument");
  if (n != 3 * c->N) return api_fail("tlfea_contact_set_base_force: n must be 3N = " + std::to_string(3 * c->N));
  HIP_TRY(hipMemcpy(c->d_base, f, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

extern "C" int tlfea_contact_apply_to_t10(tlfea_contact_t c) {
  if (!c) return api_fail("tlfea_contact_apply_to_t10: NULL context");
  if (!c->t10) return api_fail("tlfea_contact_apply_to_t10: no element object bound (tlfea_contact_bind_t10)");
  double* f_ext = tlfea_t10_external_force_device_ptr(c->t10);
  if (!f_ext) return api_fail("tlfea_contact_apply_to_t10: the element object has no external-force buffer");
  launch_contact_add(c->stream, 3 * c->N, c->d_base, c->d_force, f_ext);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// GetExternalForcesDevicePtr
extern "C" double* tlfea_contact_force_device_ptr(tlfea_contact_t c) { return c ? c->d_force : nullptr; }

// GetNumContacts
extern "C" int tlfea_contact_num_pairs(tlfea_contact_t c, int* n) {
  if (!c || !n) return api_fail("tlfea_contact_num_pairs: NULL argument");
  *n = c->n_pairs;
  return 0;
}

extern "C" int tlfea_contact_num_patches(tlfea_contact_t c, int* n) {
  if (!c || !n) return api_fail("tlfea_contact_num_patches: NULL argument");
  HIP_TRY(hipMemcpy(n, c->d_n_valid, sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

// RetrieveResults
extern "C" int tlfea_contact_retrieve_pairs(tlfea_contact_t c, int* pairs) {
  if (!c || (!pairs && c->n_pairs)) return api_fail("tlfea_contact_retrieve_pairs: NULL argument");
  if (c->n_pairs) HIP_TRY(hipMemcpy(pairs, c->d_pairs, (size_t)c->n_pairs * sizeof(int2), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int tlfea_contact_retrieve_patches(tlfea_contact_t c, tlfea_contact_patch* patches) {
  if (!c || (!patches && c->n_pairs)) return api_fail("tlfea_contact_retrieve_patches: NULL argument");
  if (c->n_pairs)
    HIP_TRY(hipMemcpy(patches, c->d_patches, (size_t)c->n_pairs * sizeof(tlfea_contact_patch),
                        hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int tlfea_contact_retrieve_force(tlfea_contact_t c, double* f) {
  if (!c || !f) return api_fail("tlfea_contact_retrieve_force: NULL argument");
  HIP_TRY(hipMemcpy(f, c->d_force, 3 * (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
