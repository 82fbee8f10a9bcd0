// test_net_identify -- Young's modulus of a welded ANCF-3243 beam net from its centre deflection alone (DESIGN 3j').  The
// 20 x 20 net of tests/golden/meshes is clamped at its four corner joints and loaded at the centre joint, as in
// test_ancf3243_net_newton; three implicit steps from rest give the centre deflection.  The "measurement" is that
// deflection computed with the true modulus.  Starting 40 % below it, the driver runs Newton's method on the scalar misfit
// r(E) = u(E) - u_measured  with du/dE from SyncedNewtonSolver::ANCFAdjointStep chained backwards through the three steps,
// and prints the iterates.  Exits non-zero when E is not recovered to 1e-6 relative in 8 iterations.
// --wrong_derivative=1 halves du/dE (the convergence a wrong derivative gives: linear, not there in 8).
//   ./test_net_identify --mesh_dir=tests/golden/meshes
#include <cmath>
#include <iomanip>
#include <memory>

#include "tlfea_facade.h"

namespace {
const double kETrue = 7e8, kNu = 0.33, kRho0 = 2700;  // test_ancf3243_net_newton
const int kSteps = 3;
bool StartsWith(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }

struct Net {
  GPU_ANCF3243_Data& data;
  SyncedNewtonSolver& solver;
  tlfea::VectorXd x0, y0, z0;
  std::vector<int> centre;  // position coefficients of the loaded joint
  int n_coef;

  // centre deflection in z after kSteps steps from rest with modulus E; with dE: also du/dE by the adjoint chain
  double Deflection(double E, double* dE) {
    const size_t n = 3 * (size_t)n_coef, nc = (size_t)data.get_n_constraint();
    data.SetSVK(E, kNu);
    data.UpdatePositions(x0, y0, z0);
    std::vector<double> zero(n, 0.0), lam0(nc, 0.0);
    TLFEA_HANDLE_ERROR(tlfea_newton_set_velocity(solver.handle(), zero.data(), zero.data()));
    TLFEA_HANDLE_ERROR(tlfea_newton_set_lambda(solver.handle(), lam0.data()));
    struct State {
      tlfea::VectorXd x, y, z;
      std::vector<double> v, lam;
    };
    std::vector<State> st(kSteps + 1);
    st[0] = State{x0, y0, z0, zero, lam0};
    for (int k = 1; k <= kSteps; k++) {
      solver.Solve();
      State& s = st[k];
      s.x.resize(n_coef); s.y.resize(n_coef); s.z.resize(n_coef);
      data.RetrievePositionToCPU(s.x, s.y, s.z);
      s.v.assign(n, 0.0);
      s.lam.assign(nc, 0.0);
      TLFEA_HANDLE_ERROR(tlfea_newton_retrieve_velocity(solver.handle(), s.v.data()));
      TLFEA_HANDLE_ERROR(tlfea_newton_retrieve_lambda(solver.handle(), s.lam.data()));
    }
    double u = 0.0;
    for (int c : centre) u += (st[kSteps].z(c) - z0(c)) / centre.size();
    if (!dE) return u;
    // cotangents of the last state: u reads the centre joint's z alone
    std::vector<double> xbar(n, 0.0), vbar(n, 0.0), lambar(nc, 0.0);
    for (int c : centre) xbar[3 * c + 2] = 1.0 / centre.size();
    double dlam = 0.0, dmu = 0.0;
    for (int k = kSteps; k >= 1; k--) {
      const State& s = st[k];
      data.UpdatePositions(s.x, s.y, s.z);
      TLFEA_HANDLE_ERROR(tlfea_newton_set_velocity(solver.handle(), s.v.data(), s.v.data()));
      TLFEA_HANDLE_ERROR(tlfea_newton_set_lambda(solver.handle(), s.lam.data()));
      const SyncedNewtonSolver::AdjointResult r = solver.ANCFAdjointStep(xbar, vbar, lambar, st[k - 1].v);
      dlam += r.per_material[0];
      dmu += r.per_material[1];
      xbar = r.x_prev;
      vbar = r.v_prev;  // the step's input velocity enters as v_prev alone
      lambar = r.lam_in;
    }
    // lambda = E nu / ((1 + nu)(1 - 2 nu)), mu = E / (2 (1 + nu)): both linear in E
    *dE = dlam * kNu / ((1 + kNu) * (1 - 2 * kNu)) + dmu / (2 * (1 + kNu));
    return u;
  }
};
}  // namespace

int main(int argc, char** argv) {
  std::string mesh_dir = "tests/golden/meshes";
  bool wrong = false;
  // the step: a tenth of a second, long against the net's first period, so three steps carry most of the static deflection
  // and u depends on E; the penalty keeps rho h^2 (1e6) well above the beams' stiffness per joint without lifting the
  // rounding floor of ||g|| (eps |x| rho h) over inner_atol
  double dt = 0.1, rho = 1e8, atol = 1e-4, force = -1000.0;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (StartsWith(a, "--mesh_dir=")) mesh_dir = a.substr(11);
    else if (StartsWith(a, "--wrong_derivative=")) wrong = std::atoi(a.c_str() + 19) != 0;
    else if (StartsWith(a, "--dt=")) dt = std::atof(a.c_str() + 5);
    else if (StartsWith(a, "--rho=")) rho = std::atof(a.c_str() + 6);
    else if (StartsWith(a, "--atol=")) atol = std::atof(a.c_str() + 7);
    else if (StartsWith(a, "--force=")) force = std::atof(a.c_str() + 8);
    else {
      std::cerr << "Unknown argument: " << a << std::endl;
      return 1;
    }
  }
  if (tlfea_device_count() <= 0) {
    std::cerr << "No HIP device visible" << std::endl;
    return 1;
  }
  ANCFCPUUtils::ANCF3243Mesh mesh;
  std::string err;
  if (!ANCFCPUUtils::ReadANCF3243MeshFromFile(mesh_dir + "/ANCF3243/net_welded_nx20_ny20_L0.5.ancf3243mesh", mesh, &err)) {
    std::cerr << err << std::endl;
    return 1;
  }
  const int n_nodes = mesh.n_nodes, n_coef = 4 * n_nodes, n_dofs = 3 * n_coef;
  double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300;
  for (int i = 0; i < n_nodes; i++) {
    xmin = std::min(xmin, mesh.x12(4 * i)); xmax = std::max(xmax, mesh.x12(4 * i));
    ymin = std::min(ymin, mesh.y12(4 * i)); ymax = std::max(ymax, mesh.y12(4 * i));
  }
  auto nodes_at = [&](double x, double y) {
    std::vector<int> out;
    for (int i = 0; i < n_nodes; i++)
      if (std::abs(mesh.x12(4 * i) - x) < 1e-9 && std::abs(mesh.y12(4 * i) - y) < 1e-9) out.push_back(i);
    return out;
  };
  const std::vector<int> centre_nodes = nodes_at(0.5 * (xmin + xmax), 0.5 * (ymin + ymax));
  if (centre_nodes.empty()) {
    std::cerr << "no joint at the net centre" << std::endl;
    return 1;
  }
  GPU_ANCF3243_Data data(n_nodes, mesh.n_elements);
  data.Initialize();
  tlfea::VectorXd f_ext(n_dofs);
  f_ext.setZero();
  std::vector<int> centre;
  for (int nd : centre_nodes) {
    f_ext((4 * nd) * 3 + 2) += force / centre_nodes.size();
    centre.push_back(4 * nd);
  }
  data.SetExternalForce(f_ext);
  data.Setup(mesh.has_grid ? mesh.grid_L : 0.5, 0.1, 0.1, Quadrature::gauss_xi_m_6, Quadrature::gauss_xi_3,
             Quadrature::gauss_eta_2, Quadrature::gauss_zeta_2, Quadrature::weight_xi_m_6, Quadrature::weight_xi_3,
             Quadrature::weight_eta_2, Quadrature::weight_zeta_2, mesh.x12, mesh.y12, mesh.z12, mesh.element_connectivity);
  data.SetDensity(kRho0);
  data.SetDamping(0.0, 0.0);
  data.SetSVK(kETrue, kNu);
  ANCFCPUUtils::LinearConstraintBuilder builder(n_dofs, mesh.constraints);
  const double corners[4][2] = {{xmin, ymin}, {xmax, ymin}, {xmin, ymax}, {xmax, ymax}};
  for (const auto& c : corners)
    for (int nd : nodes_at(c[0], c[1]))
      for (int slot = 0; slot < 4; slot++)
        ANCFCPUUtils::AppendANCF3243FixedCoefficient(builder, 4 * nd + slot, mesh.x12, mesh.y12, mesh.z12);
  const ANCFCPUUtils::LinearConstraintCSR all = builder.ToCSR();
  data.SetLinearConstraintsCSR(all.offsets, all.columns, all.values, all.rhs);
  data.CalcDsDuPre();
  data.CalcMassMatrix();
  data.CalcConstraintData();

  // one outer iteration per step (the adjoint differentiates exactly that); the direct solve, as the net's own driver
  SyncedNewtonParams params = {atol, 0.0, 1e-6, rho, 1, 20, dt};
  int rc = 0;
  {
    SyncedNewtonSolver solver(&data, data.get_n_constraint());
    solver.Setup();
    solver.SetParameters(&params);
    tlfea_linsolve_opts lin = {1e-12, 20000, 25, 0, 0.0, 0, 0, 1, 0};
    TLFEA_HANDLE_ERROR(tlfea_newton_set_linsolve_opts(solver.handle(), &lin));
    tlfea::VectorXd x0 = mesh.x12, y0 = mesh.y12, z0 = mesh.z12;
    Net net{data, solver, x0, y0, z0, centre, n_coef};
    const double u_meas = net.Deflection(kETrue, nullptr);
    std::cout << std::scientific << std::setprecision(12) << "measured centre deflection " << u_meas << " (E = " << kETrue << ")"
              << std::endl;
    double E = 0.6 * kETrue;
    bool found = false;
    for (int it = 0; it <= 8; it++) {
      double dE = 0.0;
      const double u = net.Deflection(E, &dE);
      const double rel = std::abs(E - kETrue) / kETrue;
      std::cout << "iterate " << it << ": E = " << E << " u = " << u << " du/dE = " << dE << " |E - E_true| / E_true = "
                << std::setprecision(3) << rel << std::setprecision(12) << std::endl;
      if (!std::isfinite(u) || !std::isfinite(dE) || dE == 0.0) break;
      if (rel <= 1e-6) {
        found = true;
        std::cout << "recovered in " << it << " Newton iterations" << std::endl;
        break;
      }
      if (it == 8) break;
      E -= (u - u_meas) / (wrong ? 0.5 * dE : dE);
    }
    if (!found) {
      std::cout << "not recovered in 8 Newton iterations" << std::endl;
      rc = 2;
    }
  }
  data.Destroy();
  return rc;
}
