// test_sphere_drop_collision -- lib_bin/collision_system/test_sphere_drop_collision.cc of the reference on this engine:
// a sphere falls onto a second one whose lower half is pinned; hydroelastic contact (tlfea_collision.h) -> f_ext ->
// implicit Newton step, every step on the device (Step -> ApplyToElementData -> Solve, no host round trip of forces).
//   ./test_sphere_drop_collision [damping=0.2] [friction=0.8] [self_collision=0] [steps=2500] [export_interval=5]
//                                [--mesh_dir=data/meshes/T10] [--csv_path=FILE] [--vtk_dir=output] [--gap=0.02]
// --csv_path records per step: step,top_center_z,num_pairs,num_patches,contact_fz_top (top_center_z: mean z of the top
// sphere's nodes after the step; the rest: the contact step before it).  Every 20th step prints its contact time
// (hipEvents); export_interval > 0 writes both spheres as VTU (pressure as point data) to --vtk_dir.
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "tlfea_collision.h"

namespace {
const double kE = 4e6, kNu = 0.3, kRho0 = 3500.0;  // test_sphere_drop_collision.cc:30-32
const double kGravity = -9.81, kDt = 5e-4, kRadius = 0.15;
bool starts_with(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }
}  // namespace

int main(int argc, char** argv) {
  double damping = 0.2, friction = 0.8, gap = 0.02;
  bool self_collision = false;
  int steps = 2500, export_interval = 5;
  std::string mesh_dir = "data/meshes/T10", csv_path, vtk_dir = "output";
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++) {
    const std::string a(argv[i]);
    if (starts_with(a, "--mesh_dir=")) mesh_dir = a.substr(11);
    else if (starts_with(a, "--csv_path=")) csv_path = a.substr(11);
    else if (starts_with(a, "--vtk_dir=")) vtk_dir = a.substr(10);
    else if (starts_with(a, "--gap=")) gap = std::atof(a.c_str() + 6);
    else if (starts_with(a, "--")) {
      std::cerr << "Unknown argument: " << a << std::endl;
      return 1;
    } else {
      pos.push_back(a);
    }
  }
  if (pos.size() > 5) {
    std::cerr << "Too many positional arguments (damping friction self_collision steps export_interval)" << std::endl;
    return 1;
  }
  if (pos.size() > 0) damping = std::atof(pos[0].c_str());
  if (pos.size() > 1) friction = std::atof(pos[1].c_str());
  if (pos.size() > 2) self_collision = std::atoi(pos[2].c_str()) != 0;
  if (pos.size() > 3 && std::atoi(pos[3].c_str()) > 0) steps = std::atoi(pos[3].c_str());
  if (pos.size() > 4) export_interval = std::atoi(pos[4].c_str());
  std::cout << "Contact damping: " << damping << "\nContact friction: " << friction
            << "\nSelf collision: " << (self_collision ? "on" : "off") << "\nSteps: " << steps
            << "\nExport interval: " << export_interval << std::endl;
  if (tlfea_device_count() <= 0) {
    std::cerr << "No HIP device visible" << std::endl;
    return 1;
  }

  ANCFCPUUtils::MeshManager mm;
  const std::string sphere = mesh_dir + "/sphere.1";
  const int bottom = mm.LoadMesh(sphere + ".node", sphere + ".ele", "sphere_bottom");
  const int top = mm.LoadMesh(sphere + ".node", sphere + ".ele", "sphere_top");
  if (bottom < 0 || top < 0) return 1;
  for (int m : {bottom, top})
    if (!mm.LoadScalarFieldFromNpz(m, sphere + ".uncompressed.npz", "p_vertex")) return 1;
  mm.TranslateMesh(top, 0.0, 0.0, 2.0 * kRadius + gap);  // :119-121
  const tlfea::MatrixXd& nodes = mm.GetAllNodes();
  const tlfea::MatrixXi& elements = mm.GetAllElements();
  const tlfea::VectorXd& pressure = mm.GetAllScalarFields();
  const int n_nodes = mm.GetTotalNodes(), n_elems = mm.GetTotalElements();
  const ANCFCPUUtils::MeshInstance ib = mm.GetMeshInstance(bottom), it = mm.GetMeshInstance(top);

  double zc = 0.0;  // pin the bottom sphere's nodes below its centroid (:167-195)
  for (int i = 0; i < ib.num_nodes; i++) zc += nodes(ib.node_offset + i, 2);
  zc /= ib.num_nodes;
  std::vector<int> fixed;
  for (int i = 0; i < ib.num_nodes; i++)
    if (nodes(ib.node_offset + i, 2) < zc) fixed.push_back(ib.node_offset + i);
  tlfea::VectorXi h_fixed(static_cast<int>(fixed.size()));
  for (size_t i = 0; i < fixed.size(); i++) h_fixed(static_cast<int>(i)) = fixed[i];
  std::cout << "Nodes: " << n_nodes << ", elements: " << n_elems << ", fixed: " << fixed.size() << std::endl;

  // gravity on the top sphere, spread evenly over its nodes (:361-371)
  const double mass = kRho0 * 4.0 / 3.0 * M_PI * kRadius * kRadius * kRadius;
  const double fz_node = mass / it.num_nodes * kGravity;
  tlfea::VectorXd base(3 * n_nodes);
  for (int i = 0; i < it.num_nodes; i++) base(3 * (it.node_offset + i) + 2) = fz_node;

  GPU_FEAT10_Data data(n_elems, n_nodes);
  data.Initialize();
  data.SetNodalFixed(h_fixed);
  data.SetExternalForce(base);
  tlfea::VectorXd x(n_nodes), y(n_nodes), z(n_nodes);
  for (int i = 0; i < n_nodes; i++) x(i) = nodes(i, 0), y(i) = nodes(i, 1), z(i) = nodes(i, 2);
  data.Setup(Quadrature::tet5pt_x, Quadrature::tet5pt_y, Quadrature::tet5pt_z, Quadrature::tet5pt_weights, x, y, z,
             elements);
  data.SetDensity(kRho0);
  data.SetDamping(1e4, 1e4);
  data.SetSVK(kE, kNu);
  data.CalcDnDuPre();
  data.CalcMassMatrix();
  data.CalcConstraintData();
  data.ConvertToCSR_ConstraintJacT();
  data.BuildConstraintJacobianCSR();

  SyncedNewtonParams params = {1e-8, 0.0, 1e-10, 1e12, 3, 5, kDt};  // :224
  auto solver_ptr = std::make_unique<SyncedNewtonSolver>(&data, data.get_n_constraint());
  SyncedNewtonSolver& solver = *solver_ptr;
  solver.Setup();
  solver.SetParameters(&params);

  tlfea::VectorXi mesh_ids(n_elems);
  for (int e = 0; e < n_elems; e++) mesh_ids(e) = mm.GetMeshIdFromElement(e);
  auto contact_ptr =
      std::make_unique<HydroelasticPatchCollisionSystem>(mm, nodes, elements, pressure, mesh_ids, self_collision);
  HydroelasticPatchCollisionSystem& contact = *contact_ptr;
  contact.BindElementData(&data);
  contact.SetBaseForce(base);
  CollisionSystemInput in;
  in.d_vel_xyz = solver.GetVelocityGuessDevicePtr();
  in.dt = kDt;
  const CollisionSystemParams prm{damping, friction};

  std::ofstream csv;
  if (!csv_path.empty()) {
    csv.open(csv_path);
    if (!csv) {
      std::cerr << "Cannot write " << csv_path << std::endl;
      return 1;
    }
    csv << std::setprecision(17) << "step,top_center_z,num_pairs,num_patches,contact_fz_top\n";
  }
  if (export_interval > 0 && !vtk_dir.empty()) std::filesystem::create_directories(vtk_dir);
  hipEvent_t ev0, ev1;
  if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) return 1;
  tlfea::VectorXd fc, xx, yy, zz;
  double ms_total = 0.0;
  for (int step = 0; step < steps; step++) {
    (void)hipEventRecord(ev0, nullptr);
    contact.Step(in, prm);
    contact.ApplyToElementData();
    (void)hipEventRecord(ev1, nullptr);
    (void)hipEventSynchronize(ev1);
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, ev0, ev1);
    ms_total += ms;
    const int n_pairs = contact.GetNumContacts(), n_patches = contact.GetNumPatches();
    contact.RetrieveForces(fc);
    double fz_top = 0.0;
    for (int i = 0; i < it.num_nodes; i++) fz_top += fc(3 * (it.node_offset + i) + 2);
    solver.Solve();
    data.RetrievePositionToCPU(xx, yy, zz);
    double top_z = 0.0;
    for (int i = 0; i < it.num_nodes; i++) top_z += zz(it.node_offset + i);
    top_z /= it.num_nodes;
    if (csv.is_open()) csv << step << "," << top_z << "," << n_pairs << "," << n_patches << "," << fz_top << "\n";
    if (step % 20 == 0)
      std::cout << "Step " << std::setw(4) << step << ": pairs=" << std::setw(5) << n_pairs << ", patches="
                << std::setw(4) << n_patches << ", top_z=" << std::fixed << std::setprecision(5) << top_z
                << ", |f_g|=" << std::scientific << std::setprecision(2) << std::fabs(fz_node * it.num_nodes)
                << ", f_c,z=" << fz_top << ", t_coll(ms)=" << std::fixed << std::setprecision(3) << ms << std::endl;
    if (export_interval > 0 && !vtk_dir.empty() && step % export_interval == 0) {
      tlfea::MatrixXd cur(n_nodes, 3);
      for (int n = 0; n < n_nodes; n++) cur(n, 0) = xx(n), cur(n, 1) = yy(n), cur(n, 2) = zz(n);
      ANCFCPUUtils::VisualizationUtils::ExportMeshToVTU(
          cur, elements, pressure, vtk_dir + "/sphere_drop_step_" + std::to_string(step) + ".vtu");
    }
  }
  std::cout << "Mean contact step: " << std::fixed << std::setprecision(3) << ms_total / std::max(steps, 1) << " ms"
            << std::endl;
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  contact_ptr.reset();
  solver_ptr.reset();
  data.Destroy();
  return 0;
}
