// test_beam_stress -- the cantilever of test_feat10_resolution (x = 0 clamped, 5000 N over the face x = 3, Newton steps)
// with stress recovery after every step: prints the five totals and the largest nodal von Mises stress,
// writes the last state as a VTU with nodal displacement, stress and von Mises, exits non-zero on a non-finite value.
//   ./test_beam_stress --mesh_dir=tests/golden/meshes [--res=2] [--steps=5] [--dt=1e-3] [--vtu=beam_stress.vtu]
#include <cmath>
#include <iomanip>

#include "tlfea_facade.h"
#include "tlfea_visualization.h"

namespace {
const double kE = 7e8, kNu = 0.33, kRho0 = 2700;  // test_feat10_resolution
bool StartsWith(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }
}  // namespace

int main(int argc, char** argv) {
  int res = 2, steps = 5;
  double dt = 1e-3;
  std::string mesh_dir = "data/meshes/T10/resolution", vtu = "beam_stress.vtu";
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (StartsWith(a, "--res=")) res = std::atoi(a.c_str() + 6);
    else if (StartsWith(a, "--steps=")) steps = std::atoi(a.c_str() + 8);
    else if (StartsWith(a, "--dt=")) dt = std::atof(a.c_str() + 5);
    else if (StartsWith(a, "--mesh_dir=")) mesh_dir = a.substr(11);
    else if (StartsWith(a, "--vtu=")) vtu = a.substr(6);
    else {
      std::cerr << "Unknown argument: " << a << std::endl;
      return 1;
    }
  }
  if (tlfea_device_count() <= 0) {
    std::cerr << "No HIP device visible" << std::endl;
    return 1;
  }
  tlfea::MatrixXd nodes;
  tlfea::MatrixXi elements;
  const std::string stem = mesh_dir + "/beam_3x2x1_res" + std::to_string(res) + ".1";
  const int n_nodes = ANCFCPUUtils::FEAT10_read_nodes(stem + ".node", nodes);
  const int n_elems = ANCFCPUUtils::FEAT10_read_elements(stem + ".ele", elements);
  if (!n_nodes || !n_elems) return 1;

  GPU_FEAT10_Data data(n_elems, n_nodes);
  data.Initialize();
  tlfea::VectorXd x0(n_nodes), y0(n_nodes), z0(n_nodes);
  for (int i = 0; i < n_nodes; i++) x0(i) = nodes(i, 0), y0(i) = nodes(i, 1), z0(i) = nodes(i, 2);
  std::vector<int> fixed, loaded;
  for (int i = 0; i < n_nodes; i++) {
    if (std::abs(x0(i)) < 1e-8) fixed.push_back(i);
    if (std::abs(x0(i) - 3.0) < 1e-8) loaded.push_back(i);
  }
  tlfea::VectorXi h_fixed(static_cast<int>(fixed.size()));
  for (size_t i = 0; i < fixed.size(); i++) h_fixed(static_cast<int>(i)) = fixed[i];
  data.SetNodalFixed(h_fixed);
  tlfea::VectorXd f_ext(3 * n_nodes);
  for (int n : loaded) f_ext(3 * n) = 5000.0 / loaded.size();
  data.SetExternalForce(f_ext);
  data.Setup(Quadrature::tet5pt_x, Quadrature::tet5pt_y, Quadrature::tet5pt_z, Quadrature::tet5pt_weights, x0, y0, z0,
             elements);
  data.SetDensity(kRho0);
  data.SetDamping(0.0, 0.0);
  data.SetSVK(kE, kNu);
  data.CalcDnDuPre();
  data.CalcMassMatrix();
  data.CalcConstraintData();
  data.ConvertToCSR_ConstraintJacT();
  data.BuildConstraintJacobianCSR();

  SyncedNewtonParams params = {1e-4, 1e-4, 1e-4, 1e14, 5, 10, dt};
  bool finite = true;
  tlfea::MatrixXd sigma;
  tlfea::VectorXd vm, x, y, z;
  {
    SyncedNewtonSolver solver(&data, data.get_n_constraint());
    solver.Setup();
    solver.SetParameters(&params);
    solver.AnalyzeHessianSparsity();
    solver.SetFixedSparsityPattern(true);
    for (int step = 0; step < steps; ++step) {
      solver.Solve();
      if (data.CalcStress(solver.GetVelocityGuessDevicePtr()) != 0) return 1;
      const GPU_FEAT10_Data::Energies en = data.GetEnergies();
      data.RetrieveNodalStressToCPU(sigma, vm);
      double vm_max = 0.0;
      for (int i = 0; i < n_nodes; i++) {
        vm_max = std::max(vm_max, vm(i));
        finite = finite && std::isfinite(vm(i));
      }
      for (double e : {en.strain, en.kinetic, en.viscous_power, en.reference_volume, en.current_volume})
        finite = finite && std::isfinite(e);
      std::cout << "Step " << step << std::scientific << std::setprecision(9) << ": strain=" << en.strain
                << " kinetic=" << en.kinetic << " viscous_power=" << en.viscous_power << " V0=" << en.reference_volume
                << " V=" << en.current_volume << " max_von_mises=" << vm_max << std::endl;
    }
  }
  data.RetrievePositionToCPU(x, y, z);
  tlfea::MatrixXd cur(n_nodes, 3);
  tlfea::VectorXd disp(3 * n_nodes);
  for (int i = 0; i < n_nodes; i++) {
    cur(i, 0) = x(i), cur(i, 1) = y(i), cur(i, 2) = z(i);
    disp(3 * i) = x(i) - x0(i), disp(3 * i + 1) = y(i) - y0(i), disp(3 * i + 2) = z(i) - z0(i);
    finite = finite && std::isfinite(x(i)) && std::isfinite(y(i)) && std::isfinite(z(i));
  }
  if (steps > 0 && !ANCFCPUUtils::VisualizationUtils::ExportMeshWithStress(cur, elements, disp, sigma, vm, vtu)) return 1;
  data.Destroy();
  if (!finite) {
    std::cerr << "non-finite value" << std::endl;
    return 2;
  }
  return 0;
}
