// Surface loads on a T10 block (DESIGN 3h'; no reference counterpart): a structured box of --nx x --ny x --nz cells (6 T10
// tets each, SVK 7e8 / 0.33 / 2700) clamped at x = 0, under its own weight (SetGravity) and a follower pressure on its
// top face z = lz (GetBoundaryFaces, AddFacePressure) that is ramped over the steps through the load's scale factor
// (SetFaceLoadScale).  Prints the load resultant at the undeformed mesh next to its closed form m a - p A n, then per step
// the scale, the load resultant of the step's last gradient evaluation, the deflection of the free end and the Newton
// iterations.
//   ./test_pressurized_block [--nx=4] [--ny=2] [--nz=2] [--steps=5] [--dt=1e-2] [--pressure=2e5] [--gravity=-9.81]
//                            [--max_inner=60]
#include <array>
#include <cmath>
#include <iomanip>
#include <map>
#include <memory>
#include <vector>

#include "tlfea_facade.h"

namespace {
const int kTets[6][4] = {{0, 1, 2, 6}, {0, 2, 3, 6}, {0, 3, 7, 6}, {0, 7, 4, 6}, {0, 4, 5, 6}, {0, 5, 1, 6}};
const int kCorner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
const int kEdges[6][2] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {1, 3}, {2, 3}};

// structured T10 box on the (2nx+1)(2ny+1)(2nz+1) lattice, positive orientation (mesh_utils.structured_t10_box)
void box(int nx, int ny, int nz, double lx, double ly, double lz, std::vector<double>& X, std::vector<int>& conn) {
  const int gx = 2 * nx + 1, gy = 2 * ny + 1;
  std::map<long, int> id;
  std::vector<std::array<int, 10>> lat;
  for (int k = 0; k < nz; k++)
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++)
        for (const auto& t : kTets) {
          int v[4][3];
          for (int a = 0; a < 4; a++)
            for (int d = 0; d < 3; d++) v[a][d] = 2 * (d == 0 ? i : d == 1 ? j : k) + 2 * kCorner[t[a]][d];
          long d1[3], d2[3], d3[3];
          for (int d = 0; d < 3; d++) d1[d] = v[1][d] - v[0][d], d2[d] = v[2][d] - v[0][d], d3[d] = v[3][d] - v[0][d];
          const long vol = d1[0] * (d2[1] * d3[2] - d2[2] * d3[1]) - d1[1] * (d2[0] * d3[2] - d2[2] * d3[0]) +
                           d1[2] * (d2[0] * d3[1] - d2[1] * d3[0]);
          if (vol < 0)
            for (int d = 0; d < 3; d++) std::swap(v[1][d], v[2][d]);
          std::array<int, 10> e{};
          for (int a = 0; a < 10; a++) {
            int p[3];
            for (int d = 0; d < 3; d++) p[d] = a < 4 ? v[a][d] : (v[kEdges[a - 4][0]][d] + v[kEdges[a - 4][1]][d]) / 2;
            const long key = ((long)p[2] * gy + p[1]) * gx + p[0];
            e[a] = (int)key;
            id.emplace(key, 0);
          }
          lat.push_back(e);
        }
  int n = 0;
  X.clear();
  for (auto& kv : id) {  // ascending lattice order, as the Python generator
    kv.second = n++;
    const long key = kv.first;
    X.push_back((key % gx) * (lx / (2 * nx)));
    X.push_back(((key / gx) % gy) * (ly / (2 * ny)));
    X.push_back((key / ((long)gx * gy)) * (lz / (2 * nz)));
  }
  conn.clear();
  for (const auto& e : lat)
    for (int a = 0; a < 10; a++) conn.push_back(id[e[a]]);
}
constexpr double kE = 7e8, kNu = 0.33, kRho0 = 2700;
bool starts_with(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }
}  // namespace


int main(int argc, char** argv) {
  int nx = 4, ny = 2, nz = 2, steps = 5, max_inner = 60;
  double dt = 1e-2, pressure = 2e5, gz = -9.81;
  for (int i = 1; i < argc; i++) {
    const std::string a(argv[i]);
    if (starts_with(a, "--nx=")) nx = std::atoi(a.c_str() + 5);
    else if (starts_with(a, "--ny=")) ny = std::atoi(a.c_str() + 5);
    else if (starts_with(a, "--nz=")) nz = std::atoi(a.c_str() + 5);
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
  if (nx <= 0 || ny <= 0 || nz <= 0 || steps <= 0 || !(dt > 0)) {
    std::cerr << "--nx, --ny, --nz, --steps and --dt must be positive\n";
    return 1;
  }
  if (tlfea_device_count() <= 0) {
    std::cerr << "No HIP device visible" << std::endl;
    return 1;
  }
  const double lx = 0.5 * nx, ly = 0.5 * ny, lz = 0.5 * nz;
  std::vector<double> X;
  std::vector<int> conn;
  box(nx, ny, nz, lx, ly, lz, X, conn);
  const int N = static_cast<int>(X.size()) / 3, E = static_cast<int>(conn.size()) / 10;
  tlfea::VectorXd x0(N), y0(N), z0(N);
  std::vector<int> clamp, tip;
  for (int i = 0; i < N; i++) {
    x0(i) = X[3 * i], y0(i) = X[3 * i + 1], z0(i) = X[3 * i + 2];
    if (std::fabs(x0(i)) < 1e-12) clamp.push_back(i);
    if (std::fabs(x0(i) - lx) < 1e-12) tip.push_back(i);
  }
  tlfea::MatrixXi c(E, 10);
  for (int e = 0; e < E; e++)
    for (int a = 0; a < 10; a++) c(e, a) = conn[10 * e + a];
  tlfea::VectorXi fixed(static_cast<int>(clamp.size()));
  for (size_t k = 0; k < clamp.size(); k++) fixed(static_cast<int>(k)) = clamp[k];

  GPU_FEAT10_Data data(E, N);
  data.Initialize();
  data.SetNodalFixed(fixed);
  data.Setup(Quadrature::tet5pt_x, Quadrature::tet5pt_y, Quadrature::tet5pt_z, Quadrature::tet5pt_weights, x0, y0, z0, c);
  data.SetDensity(kRho0);
  data.SetDamping(0.0, 0.0);
  data.SetSVK(kE, kNu);
  data.CalcDnDuPre();
  data.CalcMassMatrix();
  data.CalcConstraintData();
  data.ConvertToCSR_ConstraintJacT();
  data.BuildConstraintJacobianCSR();

  const GPU_FEAT10_Data::BoundaryFaces bf = data.GetBoundaryFaces(x0, y0, z0);
  std::vector<int> top;
  double area = 0.0;
  for (int k = 0; k < bf.count(); k++)
    if (bf.normal[3 * static_cast<size_t>(k) + 2] > 0.99) {
      top.push_back(k);
      area += bf.area[k];
    }
  const double scale0 = 1.0 / steps;
  if (data.SetGravity(0.0, 0.0, gz) != 0) return 1;
  const int k_press = data.AddFacePressure(top, pressure, scale0);
  if (k_press < 0) return 1;

  // the clamp's penalty term h rho c is rounded at h rho x 2.2e-16 on a clamped coordinate of size 1: rho = 1e10 keeps that
  // floor under the inner tolerance, which is 1e-8 of the load
  constexpr double kAtol = 1e-4;
  SyncedNewtonParams p = {kAtol, 0.0, 1e-6, 1e10, 1, max_inner, dt};
  auto solver_owner = std::make_unique<SyncedNewtonSolver>(&data, data.get_n_constraint());
  SyncedNewtonSolver& solver = *solver_owner;
  solver.Setup();
  solver.SetParameters(&p);

  const double mass = kRho0 * lx * ly * lz;
  std::cout << std::setprecision(17);
  std::cout << "PressurizedBlock: elements=" << E << " nodes=" << N << " boundary_faces=" << bf.count()
            << " top_faces=" << top.size() << " steps=" << steps << " dt=" << dt << " pressure=" << pressure
            << " gravity_z=" << gz << " mass=" << mass << " area=" << area << std::endl;
  double r[3], ng = 0.0;
  TLFEA_HANDLE_ERROR(tlfea_newton_eval_gradient(solver.handle(), &ng));  // the loads of the undeformed mesh
  data.GetLoadResultant(r);
  std::cout << "Reference: scale = " << scale0 << " resultant = " << r[0] << " " << r[1] << " " << r[2]
            << " expected = 0 0 " << mass * gz - scale0 * pressure * area << std::endl;

  for (int step = 0; step < steps; step++) {
    const double scale = static_cast<double>(step + 1) / steps;
    if (data.SetFaceLoadScale(k_press, scale) != 0) return 1;
    solver.Solve();
    double st[6];
    solver.GetStats(st);
    tlfea::VectorXd px, py, pz;
    data.RetrievePositionToCPU(px, py, pz);
    data.GetLoadResultant(r);
    double dz = 0.0;
    for (int i : tip) dz += (pz(i) - z0(i)) / tip.size();
    std::cout << "Step " << step + 1 << ": scale = " << scale << " resultant = " << r[0] << " " << r[1] << " " << r[2]
              << " tip dz = " << dz << " newton = " << static_cast<int>(st[1]) << " |g| = " << st[2] << std::endl;
    if (!(st[2] <= kAtol) || !std::isfinite(dz)) {
      std::cerr << "step " << step + 1 << " did not converge (|g| = " << st[2] << ")" << std::endl;
      return 2;
    }
  }
  solver_owner.reset();
  data.Destroy();
  return 0;
}
