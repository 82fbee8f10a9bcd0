// ANCF-3443 airless tire rolling onto a cleat (DESIGN 3e''; no reference counterpart): the tire and the rigid floor of
// test_tire_on_floor.cc plus a cleat, a box of 12 triangles turned into a field obstacle by RigidField::FromTriangles.  Its
// lower part lies under the floor plane, which stays a half-space (an unbounded body cannot be a field).  The floor is raised
// into the tire by --travel over the first third of the steps; then the cleat, --cleat_height above the floor, is moved
// under the tire along x from --cleat_start to 0 (UpdateFieldObstacle).  Per step the driver prints the cleat position, the
// floor's and the cleat's resultant on the tire and the sample points in contact with each; at the end it writes the sample
// points (x, y, z, gap, pressure) to --footprint_path (CSV).
//   test_tire_over_cleat [--mesh=FILE | --mesh_dir=DIR] [--footprint_path=FILE] [--travel=M] [--dt=S] [--stiffness=PA_PER_M]
//                        [--cleat_height=M] [--cleat_start=M] [--method=0|1] [steps]
// Defaults: 5e7 Pa/m, 2 mm of travel, a cleat 20 mm long and 1.5 mm high that starts 60 mm ahead, dt = 5e-4 s, 30 steps.
#include <algorithm>
#include <cmath>
#include <filesystem>
#include <iomanip>
#include <limits>
#include <memory>

#include "tlfea_facade.h"

namespace {
constexpr double kE = 1e8, kNu = 0.33, kRho0 = 2000, kEtaDamp = 5e4, kLambdaDamp = 5e4, kThicknessScale = 0.25;

bool starts_with(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }

tlfea_obstacle floor_at(double z, double stiffness, double friction) {
  tlfea_obstacle o{};
  o.kind = 0;
  o.p[2] = z;
  o.n[2] = 1.0;
  o.stiffness = stiffness;
  o.friction = friction;
  o.eps_v = 1e-3;
  return o;
}
}  // namespace

int main(int argc, char** argv) {
  std::string mesh_path, footprint = "output/tire_over_cleat/footprint.csv";
  int steps = 30, method = 1;
  double travel = 2e-3, dt = 5e-4, stiffness = 5e7, friction = 0.0, cleat_height = 1.5e-3, cleat_start = 0.06;
  for (int i = 1; i < argc; i++) {
    const std::string a(argv[i]);
    auto val = [&](const char* key) { return a.substr(std::string(key).size()); };
    try {
      if (starts_with(a, "--mesh=")) mesh_path = val("--mesh=");
      else if (starts_with(a, "--mesh_dir=")) mesh_path = val("--mesh_dir=") + "/ANCF3443/airless_tire.ancf3443mesh";
      else if (starts_with(a, "--footprint_path=")) footprint = val("--footprint_path=");
      else if (starts_with(a, "--travel=")) travel = std::stod(val("--travel="));
      else if (starts_with(a, "--dt=")) dt = std::stod(val("--dt="));
      else if (starts_with(a, "--stiffness=")) stiffness = std::stod(val("--stiffness="));
      else if (starts_with(a, "--cleat_height=")) cleat_height = std::stod(val("--cleat_height="));
      else if (starts_with(a, "--cleat_start=")) cleat_start = std::stod(val("--cleat_start="));
      else if (starts_with(a, "--method=")) method = std::stoi(val("--method="));
      else if (!a.empty() && a[0] != '-') steps = std::stoi(a);
      else {
        std::cerr << "Unknown argument: " << a << "\n";
        return 2;
      }
    } catch (...) {
      std::cerr << "Invalid value: " << a << "\n";
      return 2;
    }
  }
  if (mesh_path.empty() || !std::filesystem::exists(mesh_path)) {
    std::cerr << "Mesh file not found (--mesh=FILE or --mesh_dir=DIR): " << mesh_path << "\n";
    return 2;
  }
  if (steps < 3 || !(dt > 0.0) || !(travel > 0.0) || !(cleat_height > 0.0)) {
    std::cerr << "steps must be >= 3, --dt, --travel and --cleat_height > 0\n";
    return 2;
  }
  ANCFCPUUtils::ANCF3443Mesh mesh;
  std::string err;
  if (!ANCFCPUUtils::ReadANCF3443MeshFromFile(mesh_path, mesh, &err)) {
    std::cerr << err << "\n";
    return 2;
  }
  if (tlfea_device_count() <= 0) {
    std::cerr << "No HIP device visible" << std::endl;
    return 1;
  }
  tlfea::VectorXd H_scaled = mesh.element_H;
  for (int e = 0; e < H_scaled.size(); e++) H_scaled(e) *= kThicknessScale;

  GPU_ANCF3443_Data data(mesh.n_nodes, mesh.n_elements);
  data.Initialize();
  data.Setup(mesh.element_L, mesh.element_W, H_scaled, Quadrature::gauss_xi_m_7, Quadrature::gauss_eta_m_7,
             Quadrature::gauss_zeta_m_3, Quadrature::gauss_xi_4, Quadrature::gauss_eta_4, Quadrature::gauss_zeta_3,
             Quadrature::weight_xi_m_7, Quadrature::weight_eta_m_7, Quadrature::weight_zeta_m_3, Quadrature::weight_xi_4,
             Quadrature::weight_eta_4, Quadrature::weight_zeta_3, mesh.x12, mesh.y12, mesh.z12, mesh.element_connectivity);
  data.SetDensity(kRho0);
  data.SetDamping(kEtaDamp, kLambdaDamp);
  data.SetSVK(kE, kNu);

  // the hub: every coefficient of the innermost spoke nodes is held where it is (rows after the mesh file's own)
  const int n_dofs = 4 * mesh.n_nodes * 3;
  std::unique_ptr<ANCFCPUUtils::LinearConstraintBuilder> builder =
      mesh.constraints.Empty() ? std::make_unique<ANCFCPUUtils::LinearConstraintBuilder>(n_dofs)
                               : std::make_unique<ANCFCPUUtils::LinearConstraintBuilder>(n_dofs, mesh.constraints);
  auto radius = [&](int n) { return std::hypot(mesh.x12(4 * n), mesh.z12(4 * n)); };
  double r_min = std::numeric_limits<double>::infinity();
  for (int n = 0; n < mesh.n_nodes; n++)
    if (mesh.node_family[n] == "S") r_min = std::min(r_min, radius(n));
  int hub = 0;
  for (int n = 0; n < mesh.n_nodes; n++)
    if (mesh.node_family[n] == "S" && radius(n) - r_min <= 1e-8 * std::max(1.0, r_min)) {
      for (int slot = 0; slot < 4; slot++)
        ANCFCPUUtils::AppendANCF3243FixedCoefficient(*builder, 4 * n + slot, mesh.x12, mesh.y12, mesh.z12);
      hub++;
    }
  const ANCFCPUUtils::LinearConstraintCSR all = builder->ToCSR();
  data.SetLinearConstraintsCSR(all.offsets, all.columns, all.values, all.rhs);
  data.CalcDsDuPre();
  data.CalcMassMatrix();
  data.CalcConstraintData();

  // the floor starts just under the lowest sample point of the undeformed tire
  if (data.SetRigidObstacles({floor_at(-1e3, stiffness, friction)}) != 0) {
    std::cerr << tlfea_last_error() << std::endl;
    return 1;
  }
  tlfea::MatrixXd pts;
  data.RetrieveContactPointsToCPU(pts);
  double z_low = std::numeric_limits<double>::infinity();
  for (int i = 0; i < pts.rows(); i++) z_low = std::min(z_low, pts(i, 2));
  tlfea::VectorXd w;
  data.GetSurfacePointWeights(w);
  double area = 0.0;
  for (int i = 0; i < w.size(); i++) area += w(i);
  std::cout << std::setprecision(17) << "tire: nodes=" << mesh.n_nodes << " elements=" << mesh.n_elements << " hub_nodes=" << hub
            << " sampled_area=" << area << " lowest_point=" << z_low << "\nkappa " << stiffness << std::endl;

  SyncedNewtonParams params = {1e-4, 0.0, 1e-6, 1e12, 10, 10, dt};
  SyncedNewtonSolver solver(&data, data.get_n_constraint());
  solver.Setup();
  solver.SetParameters(&params);
  const tlfea_linsolve_opts lin = {1e-12, 20000, 25, 0, 0.0, 0, 0, method, 0};
  if (tlfea_newton_set_linsolve_opts(solver.handle(), &lin) != 0) {
    std::cerr << tlfea_last_error() << std::endl;
    return 1;
  }
  // the cleat in its own frame: 20 mm long (x), wider than the tire (y), from 20 mm under the final floor to cleat_height
  // above it; the frame's origin is the centre of its foot print on the final floor
  const double floor_end = z_low + travel, half_len = 0.01, half_wid = 0.12, depth = 0.02;
  std::vector<double> cv;
  for (int k = 0; k < 8; k++) {
    cv.push_back((k & 1) ? half_len : -half_len);
    cv.push_back((k & 2) ? half_wid : -half_wid);
    cv.push_back((k & 4) ? cleat_height : -depth);
  }
  const std::vector<int> ct = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  RigidField cleat = RigidField::FromTriangles(cv, ct, /*spacing=*/2.5e-3, stiffness);
  if (!cleat.ok) {
    std::cerr << tlfea_last_error() << std::endl;
    return 1;
  }
  cleat.pos[0] = cleat_start, cleat.pos[2] = floor_end;
  if (data.SetFieldObstacles({cleat}) != 0) {
    std::cerr << tlfea_last_error() << std::endl;
    return 1;
  }
  std::cout << "cleat: grid " << cleat.nx << " x " << cleat.ny << " x " << cleat.nz << " top " << floor_end + cleat_height
            << std::endl;
  const int press = steps / 3;
  for (int step = 0; step < steps; step++) {
    const double floor_z = z_low + travel * std::min(step + 1, press) / press;
    cleat.pos[0] = step < press ? cleat_start : cleat_start * (steps - 1 - step) / (steps - 1 - press);
    if (data.UpdateRigidObstacle(0, floor_at(floor_z, stiffness, friction)) != 0 || data.UpdateFieldObstacle(0, cleat) != 0) {
      std::cerr << tlfea_last_error() << std::endl;
      return 1;
    }
    solver.Solve();
    double r[4], c[4];
    data.GetObstacleResultant(0, r);
    data.GetFieldObstacleResultant(0, c);
    std::cout << "step " << step << " cleat_x " << cleat.pos[0] << " floor_z " << floor_z << " floor_force " << r[2]
              << " floor_points " << static_cast<int>(r[3]) << " cleat_force " << c[2] << " cleat_points "
              << static_cast<int>(c[3]) << std::endl;
  }
  data.RetrieveContactPointsToCPU(pts);
  const std::filesystem::path fp(footprint);
  if (fp.has_parent_path()) std::filesystem::create_directories(fp.parent_path());
  std::ofstream out(footprint);
  out << std::setprecision(17) << "x,y,z,gap,pressure\n";
  for (int i = 0; i < pts.rows(); i++)
    out << pts(i, 0) << "," << pts(i, 1) << "," << pts(i, 2) << "," << pts(i, 3) << "," << pts(i, 4) << "\n";
  data.Destroy();
  return 0;
}
