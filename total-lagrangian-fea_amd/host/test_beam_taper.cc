// test_beam_taper -- the thickness of a cantilever from its tip deflection alone.  The beam_3x2x1 mesh is
// clamped at x = 0 and loaded at the tip; its reference geometry is X(s) = (x, y, s z): one shape parameter s scaling the
// reference z coordinates.  Three implicit steps with a one-second time step from rest at x_0 = X(s) bring it to rest.
// The "measurement" is the mean tip deflection computed with s = 1.  Starting 20 % below it, the driver runs Newton's
// method on the scalar misfit  r(s) = u(s) - u_measured  with du/ds = sum X_bar . dX/ds from
// SyncedNewtonSolver::AdjointStep(want_shape) chained backwards through the three steps (plus the paths through the start
// x_0 = X(s), the clamped nodes' targets and the undeflected tip), and prints the iterates.  Exits non-zero when s is not
// recovered to 1e-6 relative in 8 iterations.  --wrong_derivative=1 halves du/ds (linear convergence: not there in 8).
//   ./test_beam_taper --mesh_dir=tests/golden/meshes
#include <cmath>
#include <iomanip>

#include "tlfea_facade.h"

namespace {
const double kE = 7e8, kNu = 0.33, kRho0 = 2700;  // test_feat10_resolution
const double kSTrue = 1.0;
const int kSteps = 3;
bool StartsWith(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }

struct Beam {
  GPU_FEAT10_Data& data;
  SyncedNewtonSolver& solver;
  tlfea::VectorXd x0, y0, z0;
  std::vector<int> tip, fixed;
  int n_nodes;

  // mean tip deflection in z after kSteps steps from rest with the reference z scaled by s; with ds: also du/ds
  double Deflection(double s, double* ds) {
    const size_t n = 3 * (size_t)n_nodes, nc = (size_t)data.get_n_constraint();
    tlfea::VectorXd zs(n_nodes);
    for (int i = 0; i < n_nodes; i++) zs(i) = s * z0(i);
    data.SetReferencePositions(x0, y0, zs);
    data.UpdatePositions(x0, y0, zs);
    data.UpdateConstraintTargets(x0, y0, zs);
    std::vector<double> zero(n, 0.0), lam0(nc, 0.0);
    TLFEA_HANDLE_ERROR(tlfea_newton_set_velocity(solver.handle(), zero.data(), zero.data()));
    TLFEA_HANDLE_ERROR(tlfea_newton_set_lambda(solver.handle(), lam0.data()));
    struct State {
      tlfea::VectorXd x, y, z;
      std::vector<double> v, lam;
    };
    std::vector<State> st(kSteps + 1);
    st[0] = State{x0, y0, zs, zero, lam0};
    for (int k = 1; k <= kSteps; k++) {
      solver.Solve();
      State& t = st[k];
      t.x.resize(n_nodes); t.y.resize(n_nodes); t.z.resize(n_nodes);
      data.RetrievePositionToCPU(t.x, t.y, t.z);
      t.v.assign(n, 0.0);
      t.lam.assign(nc, 0.0);
      TLFEA_HANDLE_ERROR(tlfea_newton_retrieve_velocity(solver.handle(), t.v.data()));
      TLFEA_HANDLE_ERROR(tlfea_newton_retrieve_lambda(solver.handle(), t.lam.data()));
    }
    double u = 0.0;
    for (int i : tip) u += (st[kSteps].z(i) - zs(i)) / tip.size();
    if (!ds) return u;
    // cotangents of the last state: u reads the tip's z; the undeflected tip s z0 is the direct term
    std::vector<double> xbar(n, 0.0), vbar(n, 0.0), lambar(nc, 0.0);
    double d = 0.0;
    for (int i : tip) {
      xbar[3 * i + 2] = 1.0 / tip.size();
      d -= z0(i) / tip.size();
    }
    for (int k = kSteps; k >= 1; k--) {
      const State& t = st[k];
      data.UpdatePositions(t.x, t.y, t.z);
      TLFEA_HANDLE_ERROR(tlfea_newton_set_velocity(solver.handle(), t.v.data(), t.v.data()));
      TLFEA_HANDLE_ERROR(tlfea_newton_set_lambda(solver.handle(), t.lam.data()));
      const SyncedNewtonSolver::AdjointResult r = solver.AdjointStep(xbar, vbar, lambar, false, st[k - 1].v, true);
      for (int i = 0; i < n_nodes; i++) d += r.X_bar[3 * (size_t)i + 2] * z0(i);                      // dX/ds = (0, 0, z0)
      for (size_t k2 = 0; k2 < fixed.size() && 3 * k2 + 2 < nc; k2++) d += r.targets[3 * k2 + 2] * z0(fixed[k2]);  // targets
      xbar = r.x_prev;
      vbar = r.v_prev;  // the step's input velocity enters as v_prev alone
      lambar = r.lam_in;
    }
    for (int i = 0; i < n_nodes; i++) d += xbar[3 * (size_t)i + 2] * z0(i);  // the rollout starts at x_0 = X(s)
    *ds = d;
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
  data.SetSVK(kE, kNu);
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
    Beam beam{data, solver, x0, y0, z0, tip, fixed, n_nodes};
    const double u_meas = beam.Deflection(kSTrue, nullptr);
    std::cout << std::scientific << std::setprecision(12) << "measured tip deflection " << u_meas << " (s = " << kSTrue << ")"
              << std::endl;
    double s = 0.8 * kSTrue;
    bool found = false;
    for (int it = 0; it <= 8; it++) {
      double ds = 0.0;
      const double u = beam.Deflection(s, &ds);
      const double rel = std::abs(s - kSTrue) / kSTrue;
      std::cout << "iterate " << it << ": s = " << s << " u = " << u << " du/ds = " << ds << " |s - s_true| / s_true = "
                << std::setprecision(3) << rel << std::setprecision(12) << std::endl;
      if (!std::isfinite(u) || !std::isfinite(ds) || ds == 0.0) break;
      if (rel <= 1e-6) {
        found = true;
        std::cout << "recovered in " << it << " Newton iterations" << std::endl;
        break;
      }
      if (it == 8) break;
      s -= (u - u_meas) / (wrong ? 0.5 * ds : ds);
    }
    if (!found) {
      std::cout << "not recovered in 8 Newton iterations" << std::endl;
      rc = 2;
    }
  }
  data.Destroy();
  return rc;
}
