// Distributed loads on an ANCF-3443 shell strip (no reference counterpart): the strip of test_ancf3443.cc
// (--n_beam 2 x 1 shells of thickness 0.1, SVK 7e8 / 0.33 / 2700) clamped at both short edges, under its own weight
// (SetGravity) and a follower pressure on its top face (AddFollowerPressure) that is ramped over the steps through the
// load's scale factor (SetLoadScale).  Prints the load resultant at the undeformed strip next to its closed form
// m a - p A n, then per step the scale, the load resultant of the step's last gradient evaluation, the deflection of the
// centre line and the Newton iterations.
//   ./test_shell_inflation [--n_beam=2] [--steps=10] [--dt=1.0] [--pressure=5000] [--gravity=-9.81] [--max_inner=60]
#include <cmath>
#include <iomanip>
#include <memory>

#include "tlfea_facade.h"

namespace {
constexpr double kE = 7e8, kNu = 0.33, kRho0 = 2700;
constexpr double kL = 2.0, kW = 1.0, kH = 0.1;
bool starts_with(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }
}  // namespace

int main(int argc, char** argv) {
  int n_beam = 2, steps = 10, max_inner = 60;
  double dt = 1.0, pressure = 5000.0, gz = -9.81;
  for (int i = 1; i < argc; i++) {
    const std::string a(argv[i]);
    if (starts_with(a, "--n_beam=")) n_beam = std::atoi(a.c_str() + 9);
    else if (starts_with(a, "--steps=")) steps = std::atoi(a.c_str() + 8);
    else if (starts_with(a, "--dt=")) dt = std::atof(a.c_str() + 5);
    else if (starts_with(a, "--pressure=")) pressure = std::atof(a.c_str() + 11);
    else if (starts_with(a, "--gravity=")) gz = std::atof(a.c_str() + 10);
    else if (starts_with(a, "--max_inner=")) max_inner = std::atoi(a.c_str() + 12);
    else {
      std::cerr << "Unknown argument: " << a << "\n";
      return 1;
    }
  }
  if (n_beam < 2 || n_beam % 2 || steps <= 0 || !(dt > 0)) {
    std::cerr << "--n_beam must be even and >= 2, --steps and --dt positive\n";
    return 1;
  }
  if (tlfea_device_count() <= 0) {
    std::cerr << "No HIP device visible" << std::endl;
    return 1;
  }
  GPU_ANCF3443_Data data(n_beam);  // strip constructor
  data.Initialize();
  tlfea::VectorXd x, y, z;
  tlfea::MatrixXi conn;
  ANCFCPUUtils::ANCF3443_generate_beam_coordinates(n_beam, x, y, z, conn);
  tlfea::VectorXi fixed(16);
  {
    int k = 0;
    for (int node : {conn(0, 0), conn(0, 3), conn(n_beam - 1, 1), conn(n_beam - 1, 2)})
      for (int d = 0; d < 4; d++) fixed(k++) = 4 * node + d;
  }
  data.SetNodalFixed(fixed);
  data.Setup(kL, kW, kH, Quadrature::gauss_xi_m_7, Quadrature::gauss_eta_m_7, Quadrature::gauss_zeta_m_3,
             Quadrature::gauss_xi_4, Quadrature::gauss_eta_4, Quadrature::gauss_zeta_3, Quadrature::weight_xi_m_7,
             Quadrature::weight_eta_m_7, Quadrature::weight_zeta_m_3, Quadrature::weight_xi_4, Quadrature::weight_eta_4,
             Quadrature::weight_zeta_3, x, y, z, conn);
  data.SetDensity(kRho0);
  data.SetDamping(0.0, 0.0);
  data.SetSVK(kE, kNu);
  data.CalcDsDuPre();
  data.CalcMassMatrix();
  data.CalcConstraintData();
  data.ConvertToCSR_ConstraintJacT();
  data.BuildConstraintJacobianCSR();

  std::vector<int> all(n_beam);
  for (int e = 0; e < n_beam; e++) all[e] = e;
  const double scale0 = 1.0 / steps;
  if (data.SetGravity(0.0, 0.0, gz) != 0) return 1;
  const int k_press = data.AddFollowerPressure(/*face zeta = +1*/ 1, all, pressure, scale0);
  if (k_press < 0) return 1;

  // the clamp's penalty term h rho c is rounded at h rho x 2.2e-16 on a clamped coefficient of value 1: rho = 1e10 keeps
  // that floor (1e-5 at dt = 1) under the inner tolerance, which is 1e-8 of the load
  constexpr double kAtol = 1e-4;
  SyncedNewtonParams p = {kAtol, 0.0, 1e-6, 1e10, 1, max_inner, dt};
  auto solver_owner = std::make_unique<SyncedNewtonSolver>(&data, data.get_n_constraint());
  SyncedNewtonSolver& solver = *solver_owner;
  solver.Setup();
  solver.SetParameters(&p);

  const double mass = kRho0 * n_beam * kL * kW * kH, area = n_beam * kL * kW;
  std::cout << std::setprecision(17);
  std::cout << "ShellInflation: shells=" << n_beam << " coef=" << data.get_n_coef() << " steps=" << steps << " dt=" << dt
            << " pressure=" << pressure << " gravity_z=" << gz << " mass=" << mass << " area=" << area << std::endl;
  double r[3], ng = 0.0;
  TLFEA_HANDLE_ERROR(tlfea_newton_eval_gradient(solver.handle(), &ng));  // the loads of the undeformed strip
  data.GetLoadResultant(r);
  std::cout << "Reference: scale = " << scale0 << " resultant = " << r[0] << " " << r[1] << " " << r[2]
            << " expected = 0 0 " << mass * gz - scale0 * pressure * area << std::endl;

  const int ca = 4 * conn(n_beam / 2, 0), cb = 4 * conn(n_beam / 2, 3);  // the two nodes of the centre line
  const double z0 = 0.5 * (z(ca) + z(cb));
  for (int step = 0; step < steps; step++) {
    const double scale = static_cast<double>(step + 1) / steps;
    if (data.SetLoadScale(k_press, scale) != 0) return 1;
    solver.Solve();
    double st[6];
    solver.GetStats(st);
    tlfea::VectorXd px, py, pz;
    data.RetrievePositionToCPU(px, py, pz);
    data.GetLoadResultant(r);
    std::cout << "Step " << step + 1 << ": scale = " << scale << " resultant = " << r[0] << " " << r[1] << " " << r[2]
              << " centre dz = " << 0.5 * (pz(ca) + pz(cb)) - z0 << " newton = " << static_cast<int>(st[1])
              << " |g| = " << st[2] << std::endl;
    if (!(st[2] <= kAtol) || !std::isfinite(pz(ca))) {
      std::cerr << "step " << step + 1 << " did not converge (|g| = " << st[2] << ")" << std::endl;
      return 2;
    }
  }
  solver_owner.reset();
  data.Destroy();
  return 0;
}
