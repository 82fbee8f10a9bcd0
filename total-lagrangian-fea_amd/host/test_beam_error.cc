// test_beam_error -- the ZZ error indicator over a sequence of meshes of one body (DESIGN 3f''): every mesh is clamped at
// x = 0, loaded by 2e5 N downwards (-z) spread over the nodes of the face of largest x, taken through one Newton step, and
// its stress recovered.  Prints per mesh the element count, eta_rel, the largest von Mises stress of the recovered field
// and the median element size factor for the target; exits 3 if eta_rel does not fall from one mesh to the next.
//   ./test_beam_error --mesh_dir=tests/golden/meshes [--target=0.05] [--dt=1e-3] [--vtu=last.vtu] beam_3x2x1_res2.1 beam_3x2x1_res4.1
#include <algorithm>
#include <cmath>
#include <iomanip>

#include "tlfea_facade.h"
#include "tlfea_visualization.h"

namespace {
const double kE = 7e8, kNu = 0.33, kRho0 = 2700;  // test_feat10_resolution
const double kTipLoad = -2.0e5;
bool StartsWith(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }
}  // namespace

int main(int argc, char** argv) {
  double target = 0.05, dt = 1e-3;
  std::string mesh_dir = "data/meshes/T10/resolution", vtu;
  std::vector<std::string> prefixes;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (StartsWith(a, "--target=")) target = std::atof(a.c_str() + 9);
    else if (StartsWith(a, "--dt=")) dt = std::atof(a.c_str() + 5);
    else if (StartsWith(a, "--mesh_dir=")) mesh_dir = a.substr(11);
    else if (StartsWith(a, "--vtu=")) vtu = a.substr(6);
    else if (StartsWith(a, "--")) {
      std::cerr << "Unknown argument: " << a << std::endl;
      return 1;
    } else prefixes.push_back(a);
  }
  if (prefixes.empty()) {
    std::cerr << "test_beam_error: give at least one mesh prefix (<mesh_dir>/<prefix>.node and .ele)" << std::endl;
    return 1;
  }
  if (tlfea_device_count() <= 0) {
    std::cerr << "No HIP device visible" << std::endl;
    return 1;
  }
  bool finite = true, falls = true;
  double eta_prev = 0.0;
  for (size_t k = 0; k < prefixes.size(); k++) {
    tlfea::MatrixXd nodes;
    tlfea::MatrixXi elements;
    const std::string stem = mesh_dir + "/" + prefixes[k];
    const int n_nodes = ANCFCPUUtils::FEAT10_read_nodes(stem + ".node", nodes);
    const int n_elems = ANCFCPUUtils::FEAT10_read_elements(stem + ".ele", elements);
    if (!n_nodes || !n_elems) return 1;

    GPU_FEAT10_Data data(n_elems, n_nodes);
    data.Initialize();
    tlfea::VectorXd x0(n_nodes), y0(n_nodes), z0(n_nodes);
    double x_max = nodes(0, 0);
    for (int i = 0; i < n_nodes; i++) {
      x0(i) = nodes(i, 0), y0(i) = nodes(i, 1), z0(i) = nodes(i, 2);
      x_max = std::max(x_max, x0(i));
    }
    std::vector<int> fixed, loaded;
    for (int i = 0; i < n_nodes; i++) {
      if (std::abs(x0(i)) < 1e-8) fixed.push_back(i);
      if (std::abs(x0(i) - x_max) < 1e-8) loaded.push_back(i);
    }
    tlfea::VectorXi h_fixed(static_cast<int>(fixed.size()));
    for (size_t i = 0; i < fixed.size(); i++) h_fixed(static_cast<int>(i)) = fixed[i];
    data.SetNodalFixed(h_fixed);
    tlfea::VectorXd f_ext(3 * n_nodes);
    for (int i = 0; i < 3 * n_nodes; i++) f_ext(i) = 0.0;
    for (int n : loaded) f_ext(3 * n + 2) = kTipLoad / loaded.size();
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
    {
      SyncedNewtonSolver solver(&data, data.get_n_constraint());
      solver.Setup();
      solver.SetParameters(&params);
      solver.AnalyzeHessianSparsity();
      solver.SetFixedSparsityPattern(true);
      solver.Solve();
    }
    if (data.CalcStress(nullptr, true) != 0 || data.RecoverStress(true, false) != 0) {
      std::cerr << tlfea_last_error() << std::endl;
      return 1;
    }
    tlfea::MatrixXd sigma, pn, pe;
    tlfea::VectorXd vm, eta2, n2;
    data.RetrieveRecoveredStressToCPU(sigma, vm);
    data.RetrievePrincipalStressToCPU(pn, pe);
    data.RetrieveErrorIndicatorToCPU(eta2, n2);
    const GPU_FEAT10_Data::ErrorEstimate est = data.GetErrorEstimate();
    std::vector<double> f = data.SizeFactors(target);
    std::sort(f.begin(), f.end());
    const double median = f.size() % 2 ? f[f.size() / 2] : 0.5 * (f[f.size() / 2 - 1] + f[f.size() / 2]);
    double vm_max = 0.0;
    for (int i = 0; i < n_nodes; i++) {
      vm_max = std::max(vm_max, vm(i));
      finite = finite && std::isfinite(vm(i));
    }
    finite = finite && std::isfinite(est.eta_rel) && std::isfinite(median);
    std::cout << "Mesh " << prefixes[k] << ": elements=" << n_elems << std::scientific << std::setprecision(9)
              << " eta_rel=" << est.eta_rel << " max_von_mises=" << vm_max << " median_size_factor=" << median
              << " clamped=" << est.clamped << std::endl;
    if (k > 0 && !(est.eta_rel < eta_prev)) falls = false;
    eta_prev = est.eta_rel;
    if (k + 1 == prefixes.size() && !vtu.empty()) {
      tlfea::VectorXd x, y, z;
      data.RetrievePositionToCPU(x, y, z);
      tlfea::MatrixXd cur(n_nodes, 3);
      for (int i = 0; i < n_nodes; i++) cur(i, 0) = x(i), cur(i, 1) = y(i), cur(i, 2) = z(i);
      if (!ANCFCPUUtils::VisualizationUtils::ExportMeshWithRecoveredStress(cur, elements, sigma, vm, pn, eta2, vtu)) return 1;
    }
    data.Destroy();
  }
  if (!finite) {
    std::cerr << "non-finite value" << std::endl;
    return 2;
  }
  if (!falls) {
    std::cerr << "eta_rel does not fall from one mesh to the next" << std::endl;
    return 3;
  }
  return 0;
}
