// Series bar of two materials in one GPU_FEAT10_Data (per-element materials; no reference counterpart).
// A 2 x 1 x 1 box of 4 x 2 x 2 cells (6 T10 tets each), split at x = 1 on element faces: SVK with nu = 0, E = 1e7 on
// the left half and 1e8 on the right.  Each half gets the axial stretch lam_i that makes P11 = E_i lam_i (lam_i^2 - 1) / 2
// the same in both, so every node off the end faces carries f_int = 0 -- the interface plane's nodes included -- and
// the end faces carry equal and opposite totals.  Prints interior_max=, end_force= and end_sum= (|left + right|).
#include <cmath>
#include <cstdio>
#include <array>
#include <map>
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
}  // namespace

int main() {
  std::vector<double> X;
  std::vector<int> conn;
  box(4, 2, 2, 2.0, 1.0, 1.0, X, conn);
  const int N = (int)X.size() / 3, E = (int)conn.size() / 10;
  const double E1 = 1e7, E2 = 1e8, lam1 = 1.01;
  const double p = E1 * (lam1 * lam1 - 1) / 2 * lam1;
  double lam2 = 1.0;
  for (int it = 0; it < 60; it++) lam2 -= (E2 * (lam2 * lam2 * lam2 - lam2) / 2 - p) / (E2 * (3 * lam2 * lam2 - 1) / 2);

  tlfea::VectorXd x0(N), y0(N), z0(N), x(N), y(N), z(N);
  for (int i = 0; i < N; i++) {
    x0(i) = X[3 * i];
    y0(i) = y(i) = X[3 * i + 1];
    z0(i) = z(i) = X[3 * i + 2];
    x(i) = x0(i) <= 1.0 ? lam1 * x0(i) : lam1 + lam2 * (x0(i) - 1.0);
  }
  tlfea::MatrixXi c(E, 10);
  std::vector<int> ids(E);
  for (int e = 0; e < E; e++) {
    double cx = 0.0;
    for (int a = 0; a < 10; a++) c(e, a) = conn[10 * e + a];
    for (int a = 0; a < 4; a++) cx += 0.25 * X[3 * conn[10 * e + a]];
    ids[e] = cx > 1.0 ? 1 : 0;
  }

  GPU_FEAT10_Data data(E, N);
  data.Initialize();
  data.Setup(Quadrature::tet5pt_x, Quadrature::tet5pt_y, Quadrature::tet5pt_z, Quadrature::tet5pt_weights, x0, y0, z0, c);
  std::vector<tlfea_material_entry> mats(2);
  mats[0] = tlfea_material_entry{E1, 0.0, 0.0, 0.0, 0.0, 1000.0, 0.0, 0.0};
  mats[1] = tlfea_material_entry{E2, 0.0, 0.0, 0.0, 0.0, 1000.0, 0.0, 0.0};
  if (data.SetElementMaterials(ids, mats, 0) != 0) {
    std::fprintf(stderr, "SetElementMaterials: %s\n", tlfea_last_error());
    return 1;
  }
  data.CalcDnDuPre();
  data.CalcMassMatrix();
  data.UpdatePositions(x, y, z);
  data.CalcP();
  data.CalcInternalForce();
  tlfea::VectorXd f;
  data.RetrieveInternalForceToCPU(f);
  double interior = 0.0, left[3] = {0, 0, 0}, right[3] = {0, 0, 0};
  for (int i = 0; i < N; i++) {
    const bool l = std::fabs(x0(i)) < 1e-12, r = std::fabs(x0(i) - 2.0) < 1e-12;
    for (int d = 0; d < 3; d++) {
      if (l) left[d] += f(3 * i + d);
      else if (r) right[d] += f(3 * i + d);
      else interior = std::fmax(interior, std::fabs(f(3 * i + d)));
    }
  }
  const double end = std::sqrt(right[0] * right[0] + right[1] * right[1] + right[2] * right[2]);
  const double sum = std::sqrt(std::pow(left[0] + right[0], 2) + std::pow(left[1] + right[1], 2) +
                               std::pow(left[2] + right[2], 2));
  std::printf("two_material_bar: nodes=%d elements=%d lam1=%.6f lam2=%.9f\n", N, E, lam1, lam2);
  std::printf("interior_max=%.6e end_force=%.15e end_sum=%.6e\n", interior, end, sum);
  data.Destroy();
  return (end > 0.0 && interior <= 1e-10 * end && sum <= 1e-10 * end) ? 0 : 2;
}
