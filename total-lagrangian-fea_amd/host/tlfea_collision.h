// tlfea_collision.h -- HydroelasticPatchCollisionSystem of the reference (lib_src/collision/
// HydroelasticPatchCollisionSystem.h, CollisionSystemBase.h) over the tlfea_contact_* C-ABI: same class, struct and
// member names.  Broadphase, narrowphase and the nodal forces run on the GPU (csrc/contact_kernels.hip).
// Deviation: BindElementData(GPU_FEAT10_Data*) binds the element object's own x / y / z buffers (this engine keeps
// them in separate allocations), and ApplyToElementData() writes f_ext = base + contact force on the device, so that a
// driver loop Step -> ApplyToElementData -> Solve never goes through the host.
#pragma once
#include <vector>

#include "tlfea_facade.h"

struct CollisionSystemInput {  // CollisionSystemBase.h
  double* d_nodes_xyz = nullptr;  // [x..., y..., z...] on the device, or nullptr when positions are bound already
  int n_nodes = 0;
  double* d_vel_xyz = nullptr;    // 3N interleaved velocities on the device, or nullptr
  double dt = 0.0;
};

struct CollisionSystemParams {  // CollisionSystemBase.h
  double damping = 0.0;
  double friction = 0.0;
};

using ContactPatch = tlfea_contact_patch;

class HydroelasticPatchCollisionSystem {
 public:
  // elements: E x 10 (or E x 4) node ids; pressure: one value per node; elementMeshIds: one per element (empty: taken
  // from the mesh manager)
  HydroelasticPatchCollisionSystem(const ANCFCPUUtils::MeshManager& mesh_manager, const tlfea::MatrixXd& initial_nodes,
                                   const tlfea::MatrixXi& elements, const tlfea::VectorXd& pressure,
                                   const tlfea::VectorXi& elementMeshIds, bool enable_self_collision)
      : n_nodes_(initial_nodes.rows()) {
    if (pressure.size() != n_nodes_ || (elements.cols() != 10 && elements.cols() != 4)) {
      std::fprintf(stderr, "HydroelasticPatchCollisionSystem: %d pressure values for %d nodes, %d nodes per element "
                           "(needs one value per node and 10 or 4 nodes per element)\n",
                   pressure.size(), n_nodes_, elements.cols());
      std::exit(EXIT_FAILURE);
    }
    std::vector<int> mesh(elements.rows());
    for (int e = 0; e < elements.rows(); e++)
      mesh[e] = elementMeshIds.size() == elements.rows() ? elementMeshIds(e) : mesh_manager.GetMeshIdFromElement(e);
    TLFEA_HANDLE_ERROR(tlfea_contact_create(n_nodes_, elements.rows(), elements.cols(), elements.data(),
                                            pressure.data(), mesh.data(), enable_self_collision ? 1 : 0, &h_));
  }
  ~HydroelasticPatchCollisionSystem() {
    if (h_) tlfea_contact_destroy(h_);
  }
  HydroelasticPatchCollisionSystem(const HydroelasticPatchCollisionSystem&) = delete;
  HydroelasticPatchCollisionSystem& operator=(const HydroelasticPatchCollisionSystem&) = delete;

  void BindNodesDevicePtr(double* d_nodes_xyz, int n_nodes) {
    TLFEA_HANDLE_ERROR(tlfea_contact_bind_nodes(h_, d_nodes_xyz, n_nodes));
  }
  void BindElementData(GPU_FEAT10_Data* data) { TLFEA_HANDLE_ERROR(tlfea_contact_bind_t10(h_, data->h)); }

  void Step(const CollisionSystemInput& in, const CollisionSystemParams& params) {
    if (in.d_nodes_xyz) BindNodesDevicePtr(in.d_nodes_xyz, in.n_nodes ? in.n_nodes : n_nodes_);
    TLFEA_HANDLE_ERROR(tlfea_contact_step(h_, in.d_vel_xyz, params.damping, params.friction));
  }
  void SetBaseForce(const tlfea::VectorXd& f) {
    TLFEA_HANDLE_ERROR(tlfea_contact_set_base_force(h_, f.data(), f.size()));
  }
  void ApplyToElementData() { TLFEA_HANDLE_ERROR(tlfea_contact_apply_to_t10(h_)); }

  const double* GetExternalForcesDevicePtr() const { return tlfea_contact_force_device_ptr(h_); }
  int GetNumContacts() const {
    int n = 0;
    TLFEA_HANDLE_ERROR(tlfea_contact_num_pairs(h_, &n));
    return n;
  }
  int GetNumPatches() const {
    int n = 0;
    TLFEA_HANDLE_ERROR(tlfea_contact_num_patches(h_, &n));
    return n;
  }

  // for visualization / debugging: pairs and patches of the last step to the host
  void RetrieveResults() {
    const int n = GetNumContacts();
    pairs_.assign(2 * static_cast<size_t>(n), 0);
    patches_.assign(n, ContactPatch());
    TLFEA_HANDLE_ERROR(tlfea_contact_retrieve_pairs(h_, pairs_.data()));
    TLFEA_HANDLE_ERROR(tlfea_contact_retrieve_patches(h_, patches_.data()));
  }
  std::vector<ContactPatch> GetValidPatches() const {
    std::vector<ContactPatch> out;
    for (const ContactPatch& p : patches_)
      if (p.isValid) out.push_back(p);
    return out;
  }
  const std::vector<int>& GetPairs() const { return pairs_; }
  void RetrieveForces(tlfea::VectorXd& f) const {
    f.resize(3 * n_nodes_);
    TLFEA_HANDLE_ERROR(tlfea_contact_retrieve_force(h_, f.data()));
  }

 private:
  int n_nodes_ = 0;
  tlfea_contact_t h_ = nullptr;
  std::vector<int> pairs_;
  std::vector<ContactPatch> patches_;
};
