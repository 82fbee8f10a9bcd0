// test_sphere_drop_rigid_floor -- the sphere.1 mesh dropped onto a rigid half-space (the floor z = 0) under gravity,
// implicit Newton steps with the floor's contact inside the Newton iteration.  No reference counterpart: the
// reference meshes and pins a floor slab and pushes on the body with explicit hydroelastic forces instead.
//   ./test_sphere_drop_rigid_floor [steps=300] [export_interval=0] [--mesh_dir=data/meshes/T10] [--csv_path=FILE]
//                                  [--vtk_dir=output] [--gap=0.02] [--stiffness=1e8] [--friction=0.0]
// --csv_path records per step: time,min_z,floor_fz,newton_iters,cg_iters (min_z: lowest node after the step, floor_fz:
// the floor's normal force on the sphere at the end of the step).  export_interval > 0 writes the sphere as VTU.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "tlfea_facade.h"
#include "tlfea_mesh_manager.h"
#include "tlfea_visualization.h"

namespace {
const double kE = 4e6, kNu = 0.3, kRho0 = 3500.0;  // the sphere of test_sphere_drop_collision
const double kGravity = -9.81, kDt = 1e-2;
bool starts_with(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }
}  // namespace

int main(int argc, char** argv) {
  double gap = 0.02, stiffness = 1e8, friction = 0.0;
  int steps = 300, export_interval = 0;
  std::string mesh_dir = "data/meshes/T10", csv_path, vtk_dir = "output";
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++) {
    const std::string a(argv[i]);
    if (starts_with(a, "--mesh_dir=")) mesh_dir = a.substr(11);
    else if (starts_with(a, "--csv_path=")) csv_path = a.substr(11);
    else if (starts_with(a, "--vtk_dir=")) vtk_dir = a.substr(10);
    else if (starts_with(a, "--gap=")) gap = std::atof(a.c_str() + 6);
    else if (starts_with(a, "--stiffness=")) stiffness = std::atof(a.c_str() + 12);
    else if (starts_with(a, "--friction=")) friction = std::atof(a.c_str() + 11);
    else if (starts_with(a, "--")) {
      std::cerr << "Unknown argument: " << a << std::endl;
      return 1;
    } else {
      pos.push_back(a);
    }
  }
  if (pos.size() > 2) {
    std::cerr << "Too many positional arguments (steps export_interval)" << std::endl;
    return 1;
  }
  if (pos.size() > 0 && std::atoi(pos[0].c_str()) > 0) steps = std::atoi(pos[0].c_str());
  if (pos.size() > 1) export_interval = std::atoi(pos[1].c_str());
  if (tlfea_device_count() <= 0) {
    std::cerr << "No HIP device visible" << std::endl;
    return 1;
  }

  ANCFCPUUtils::MeshManager mm;
  const std::string sphere = mesh_dir + "/sphere.1";
  const int id = mm.LoadMesh(sphere + ".node", sphere + ".ele", "sphere");
  if (id < 0) return 1;
  const tlfea::MatrixXd& nodes0 = mm.GetAllNodes();
  double zmin = nodes0(0, 2);
  for (int i = 0; i < mm.GetTotalNodes(); i++) zmin = std::min(zmin, nodes0(i, 2));
  mm.TranslateMesh(id, 0.0, 0.0, gap - zmin);  // lowest node `gap` above the floor
  const tlfea::MatrixXd& nodes = mm.GetAllNodes();
  const tlfea::MatrixXi& elements = mm.GetAllElements();
  const int n_nodes = mm.GetTotalNodes(), n_elems = mm.GetTotalElements();

  GPU_FEAT10_Data data(n_elems, n_nodes);
  data.Initialize();
  tlfea::VectorXd x(n_nodes), y(n_nodes), z(n_nodes);
  for (int i = 0; i < n_nodes; i++) x(i) = nodes(i, 0), y(i) = nodes(i, 1), z(i) = nodes(i, 2);
  data.Setup(Quadrature::tet5pt_x, Quadrature::tet5pt_y, Quadrature::tet5pt_z, Quadrature::tet5pt_weights, x, y, z,
             elements);
  data.SetDensity(kRho0);
  data.SetDamping(1e4, 1e4);
  data.SetSVK(kE, kNu);
  data.CalcDnDuPre();
  data.CalcMassMatrix();
  // gravity with the consistent nodal masses: f_ext = (row sums of M) g
  std::vector<int> off, cols;
  std::vector<double> vals;
  data.RetrieveMassCSRToCPU(off, cols, vals);
  tlfea::VectorXd fext(3 * n_nodes);
  double weight = 0.0;
  for (int i = 0; i < n_nodes; i++) {
    double m = 0.0;
    for (int k = off[i]; k < off[i + 1]; k++) m += vals[k];
    fext(3 * i + 2) = m * kGravity;
    weight -= m * kGravity;
  }
  data.SetExternalForce(fext);
  tlfea_obstacle floor{};
  floor.kind = 0;
  floor.n[2] = 1.0;
  floor.stiffness = stiffness;
  floor.friction = friction;
  floor.eps_v = 1e-3;
  if (data.SetRigidObstacles({floor}) != 0) {
    std::cerr << tlfea_last_error() << std::endl;
    return 1;
  }
  std::cout << "Nodes: " << n_nodes << ", elements: " << n_elems << "\nSteps: " << steps << ", dt: " << kDt
            << "\nFloor stiffness: " << stiffness << " Pa/m, friction: " << friction << std::endl;
  std::cout << "weight " << std::setprecision(17) << weight << std::endl;

  SyncedNewtonParams params = {1e-6, 0.0, 1e-6, 1e12, 1, 20, kDt};
  auto solver_ptr = std::make_unique<SyncedNewtonSolver>(&data, 0);
  SyncedNewtonSolver& solver = *solver_ptr;
  solver.Setup();
  solver.SetParameters(&params);

  std::ofstream csv;
  if (!csv_path.empty()) {
    csv.open(csv_path);
    if (!csv) {
      std::cerr << "Cannot write " << csv_path << std::endl;
      return 1;
    }
    csv << std::setprecision(17) << "time,min_z,floor_fz,newton_iters,cg_iters\n";
  }
  if (export_interval > 0 && !vtk_dir.empty()) std::filesystem::create_directories(vtk_dir);
  tlfea::VectorXd xx, yy, zz, pressure(n_nodes);
  for (int step = 0; step < steps; step++) {
    solver.Solve();
    double st[6], res[4];
    solver.GetStats(st);
    data.GetObstacleResultant(0, res);
    data.RetrievePositionToCPU(xx, yy, zz);
    double lowest = zz(0);
    for (int i = 1; i < n_nodes; i++) lowest = std::min(lowest, zz(i));
    const double t = (step + 1) * kDt;
    if (csv.is_open()) csv << t << "," << lowest << "," << res[2] << "," << st[1] << "," << st[4] << "\n";
    if (step % 20 == 0)
      std::cout << "Step " << std::setw(4) << step << ": min_z=" << std::scientific << std::setprecision(4) << lowest
                << ", f_floor,z=" << res[2] << " (weight " << weight << "), contacts=" << static_cast<int>(res[3])
                << ", newton=" << static_cast<int>(st[1]) << ", cg=" << static_cast<int>(st[4]) << std::endl;
    if (export_interval > 0 && !vtk_dir.empty() && step % export_interval == 0) {
      tlfea::MatrixXd cur(n_nodes, 3);
      for (int n = 0; n < n_nodes; n++) cur(n, 0) = xx(n), cur(n, 1) = yy(n), cur(n, 2) = zz(n);
      ANCFCPUUtils::VisualizationUtils::ExportMeshToVTU(cur, elements, pressure,
                                                        vtk_dir + "/sphere_floor_step_" + std::to_string(step) + ".vtu");
    }
  }
  solver_ptr.reset();
  data.Destroy();
  return 0;
}
