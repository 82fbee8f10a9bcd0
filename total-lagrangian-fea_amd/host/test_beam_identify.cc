// test_beam_identify -- Young's modulus of a cantilever from its tip deflection alone.  The beam_3x2x1 mesh
// is clamped at x = 0 and loaded at the tip; three implicit steps with a one-second time step bring it to rest.  The
// "measurement" is the mean tip deflection computed with the true modulus.  Starting 40 % below it, the driver runs
// Newton's method on the scalar misfit  r(E) = u(E) - u_measured  with du/dE from SyncedNewtonSolver::AdjointStep chained
// backwards through the three steps, and prints the iterates.  Exits non-zero when E is not recovered to 1e-6 relative
// in 8 iterations.  --wrong_derivative=1 halves du/dE (the convergence a wrong derivative gives: linear, not there in 8).
//   ./test_beam_identify --mesh_dir=tests/golden/meshes
#include <cmath>
#include <iomanip>

#include "tlfea_facade.h"

namespace {
const double kETrue = 7e8, kNu = 0.33, kRho0 = 2700;  // test_feat10_resolution
const int kSteps = 3;
bool StartsWith(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }

struct Beam {
  GPU_FEAT10_Data& data;
  SyncedNewtonSolver& solver;
  tlfea::VectorXd x0, y0, z0;
  std::vector<int> tip;
  int n_nodes;

  // mean tip deflection in z after kSteps steps from rest with modulus E; with dE: also du/dE by the adjoint chain
  double Deflection(double E, double* dE) {
    const size_t n = 3 * (size_t)n_nodes, nc = (size_t)data.get_n_constraint();
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
      s.x.resize(n_nodes); s.y.resize(n_nodes); s.z.resize(n_nodes);
      data.RetrievePositionToCPU(s.x, s.y, s.z);
      s.v.assign(n, 0.0);
      s.lam.assign(nc, 0.0);
      TLFEA_HANDLE_ERROR(tlfea_newton_retrieve_velocity(solver.handle(), s.v.data()));
      TLFEA_HANDLE_ERROR(tlfea_newton_retrieve_lambda(solver.handle(), s.lam.data()));
    }
    double u = 0.0;
    for (int i : tip) u += (st[kSteps].z(i) - z0(i)) / tip.size();
    if (!dE) return u;
    // cotangents of the last state: u reads the tip's z alone
    std::vector<double> xbar(n, 0.0), vbar(n, 0.0), lambar(nc, 0.0);
    for (int i : tip) xbar[3 * i + 2] = 1.0 / tip.size();
    double dlam = 0.0, dmu = 0.0;
    for (int k = kSteps; k >= 1; k--) {
      const State& s = st[k];
      data.UpdatePositions(s.x, s.y, s.z);
      TLFEA_HANDLE_ERROR(tlfea_newton_set_velocity(solver.handle(), s.v.data(), s.v.data()));
      TLFEA_HANDLE_ERROR(tlfea_newton_set_lambda(solver.handle(), s.lam.data()));
      const SyncedNewtonSolver::AdjointResult r = solver.AdjointStep(xbar, vbar, lambar, false, st[k - 1].v);
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
  std::string mesh_dir = "data/meshes/T10/resolution";
  bool wrong = false;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (StartsWith(a, "--mesh_dir=")) mesh_dir = a.substr(11);
    else if (StartsWith(a, "--wrong_derivative=")) wrong = std::atoi(a.c_str() + 19) != 0;
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
  const std::string stem = mesh_dir + "/beam_3x2x1.1";
  const int n_nodes = ANCFCPUUtils::FEAT10_read_nodes(stem + ".node", nodes);
  const int n_elems = ANCFCPUUtils::FEAT10_read_elements(stem + ".ele", elements);
  if (!n_nodes || !n_elems) return 1;

  GPU_FEAT10_Data data(n_elems, n_nodes);
  data.Initialize();
  tlfea::VectorXd x0(n_nodes), y0(n_nodes), z0(n_nodes);
  double x_max = 0.0;
  for (int i = 0; i < n_nodes; i++) x0(i) = nodes(i, 0), y0(i) = nodes(i, 1), z0(i) = nodes(i, 2), x_max = std::max(x_max, x0(i));
  std::vector<int> fixed, tip;
  for (int i = 0; i < n_nodes; i++) {
    if (std::abs(x0(i)) < 1e-8) fixed.push_back(i);
    if (std::abs(x0(i) - x_max) < 1e-8) tip.push_back(i);
  }
  tlfea::VectorXi h_fixed(static_cast<int>(fixed.size()));
  for (size_t i = 0; i < fixed.size(); i++) h_fixed(static_cast<int>(i)) = fixed[i];
  data.SetNodalFixed(h_fixed);
  tlfea::VectorXd f_ext(3 * n_nodes);
  f_ext.setZero();
  for (int i : tip) f_ext(3 * i + 2) = -2.0e5 / tip.size();
  data.SetExternalForce(f_ext);
  data.Setup(Quadrature::tet5pt_x, Quadrature::tet5pt_y, Quadrature::tet5pt_z, Quadrature::tet5pt_weights, x0, y0, z0,
             elements);
  data.SetDensity(kRho0);
  data.SetDamping(0.0, 0.0);
  data.SetSVK(kETrue, kNu);
  data.CalcDnDuPre();
  data.CalcMassMatrix();
  data.CalcConstraintData();
  data.ConvertToCSR_ConstraintJacT();
  data.BuildConstraintJacobianCSR();

  // one outer iteration per step (the adjoint differentiates exactly that); ||g|| stops at a rounding floor of ~5e-6
  SyncedNewtonParams params = {1e-4, 0.0, 1e-6, 1e10, 1, 20, 1.0};
  int rc = 0;
  {
    SyncedNewtonSolver solver(&data, data.get_n_constraint());
    solver.Setup();
    solver.SetParameters(&params);
    Beam beam{data, solver, x0, y0, z0, tip, n_nodes};
    const double u_meas = beam.Deflection(kETrue, nullptr);
    std::cout << std::scientific << std::setprecision(12) << "measured tip deflection " << u_meas << " (E = " << kETrue << ")"
              << std::endl;
    double E = 0.6 * kETrue;
    bool found = false;
    for (int it = 0; it <= 8; it++) {
      double dE = 0.0;
      const double u = beam.Deflection(E, &dE);
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
