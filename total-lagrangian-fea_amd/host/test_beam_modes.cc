// test_beam_modes -- natural frequencies of the clamped cantilever of test_feat10_resolution (x = 0 clamped, no load, at
// rest): SyncedNewtonSolver::ModalAnalysis for six modes, prints them in Hz and writes the mode shapes as a
// VTU (one vector point field per mode, the frequencies as field data); exits non-zero on a non-finite value.
//   ./test_beam_modes --mesh_dir=tests/golden/meshes [--res=4] [--modes=6] [--vtu=beam_modes.vtu]
#include <cmath>
#include <iomanip>

#include "tlfea_facade.h"
#include "tlfea_visualization.h"

namespace {
const double kE = 7e8, kNu = 0.33, kRho0 = 2700;  // test_feat10_resolution
bool StartsWith(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }
}  // namespace

int main(int argc, char** argv) {
  int res = 4, n_modes = 6;
  std::string mesh_dir = "data/meshes/T10/resolution", vtu = "beam_modes.vtu";
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (StartsWith(a, "--res=")) res = std::atoi(a.c_str() + 6);
    else if (StartsWith(a, "--modes=")) n_modes = std::atoi(a.c_str() + 8);
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
  std::vector<int> fixed;
  for (int i = 0; i < n_nodes; i++)
    if (std::abs(x0(i)) < 1e-8) fixed.push_back(i);
  tlfea::VectorXi h_fixed(static_cast<int>(fixed.size()));
  for (size_t i = 0; i < fixed.size(); i++) h_fixed(static_cast<int>(i)) = fixed[i];
  data.SetNodalFixed(h_fixed);
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

  SyncedNewtonParams params = {1e-4, 1e-4, 1e-4, 1e14, 5, 10, 1e-3};
  bool finite = true;
  {
    SyncedNewtonSolver solver(&data, data.get_n_constraint());
    solver.Setup();
    solver.SetParameters(&params);
    const SyncedNewtonSolver::ModalResult r = solver.ModalAnalysis(n_modes);
    std::cout << "LOBPCG: " << r.iterations << " iterations, block of " << r.block << ", " << r.converged << " of " << n_modes
              << " modes converged" << std::endl;
    for (int k = 0; k < n_modes; k++) {
      finite = finite && std::isfinite(r.freq_hz[k]) && std::isfinite(r.residuals[k]);
      std::cout << "Mode " << k << std::scientific << std::setprecision(9) << ": f=" << r.freq_hz[k] << " Hz omega2=" << r.omega2[k]
                << " residual=" << std::setprecision(3) << r.residuals[k] << std::endl;
    }
    if (!ANCFCPUUtils::VisualizationUtils::ExportModeShapesToVTU(nodes, elements, r.modes, r.freq_hz, vtu)) return 1;
  }
  data.Destroy();
  if (!finite) {
    std::cerr << "non-finite value" << std::endl;
    return 2;
  }
  return 0;
}
