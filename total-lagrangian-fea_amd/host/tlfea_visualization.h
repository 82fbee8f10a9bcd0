// tlfea_visualization.h -- the VTU exporters the reference drivers call for eyeballing results
// (lib_utils/visualization_utils.h:491-589 ExportMeshToVTU, :718-846 ExportMeshWithDisplacement,
// :848-955 ExportANCF3443ToVTU, :974-1097 ExportANCF3243ToVTU).  Same static member names / argument order under
// ANCFCPUUtils::VisualizationUtils, same ASCII UnstructuredGrid layout (precision 15, scientific) so that ParaView
// states written for the reference's files open these.  One emitter serves all of them: a writer hands it the points,
// the cells (fixed arity) and optional point data.  The contact-patch exporters (VTP/CSV/JSON) of the collision subsystem
// are not built: RetrieveResults / GetValidPatches of tlfea_collision.h hand the patches to the host.  Included by tlfea_facade.h.
#pragma once
#include <array>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

namespace ANCFCPUUtils {

struct VisualizationUtils {
  using P3 = std::array<double, 3>;
  struct PointField {
    std::string name;
    int components;
    std::vector<double> values;  // n_points * components
  };

  // points, cells of `arity` point ids each (ids relative to `points`), VTK cell type (1 vertex, 10 tetra, 12 hexahedron)
  struct Piece {
    std::vector<P3> points;
    std::vector<int> cells;
    int arity, vtk_type;
    std::vector<PointField> fields;
    std::vector<PointField> cell_fields = {};  // one tuple per cell (<CellData>)
  };
  static bool WriteVTU(const std::string& filename, const std::vector<P3>& points, const std::vector<int>& cells,
                       int arity, int vtk_type, const std::vector<PointField>& fields = {}) {
    return WriteVTU(filename, std::vector<Piece>{Piece{points, cells, arity, vtk_type, fields}});
  }
  // one <Piece> per entry, in order; field_data: arrays that belong to the whole file (<FieldData>, one tuple per value)
  static bool WriteVTU(const std::string& filename, const std::vector<Piece>& pieces,
                       const std::vector<PointField>& field_data = {}) {
    std::ofstream file(filename);
    if (!file.is_open()) {
      std::cerr << "Error: Cannot open file " << filename << " for writing" << std::endl;
      return false;
    }
    file << std::setprecision(15) << std::scientific;
    file << "<?xml version=\"1.0\"?>\n"
         << "<VTKFile type=\"UnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\">\n"
         << "  <UnstructuredGrid>\n";
    if (!field_data.empty()) {
      file << "    <FieldData>\n";
      for (const PointField& f : field_data) {
        file << "      <DataArray type=\"Float64\" Name=\"" << f.name << "\" NumberOfTuples=\"" << f.values.size()
             << "\" format=\"ascii\">\n         ";
        for (double v : f.values) file << " " << v;
        file << "\n      </DataArray>\n";
      }
      file << "    </FieldData>\n";
    }
    for (const Piece& p : pieces) write_piece(file, p.points, p.cells, p.arity, p.vtk_type, p.fields, p.cell_fields);
    file << "  </UnstructuredGrid>\n</VTKFile>\n";
    return static_cast<bool>(file);
  }
  static void write_piece(std::ofstream& file, const std::vector<P3>& points, const std::vector<int>& cells, int arity,
                          int vtk_type, const std::vector<PointField>& fields,
                          const std::vector<PointField>& cell_fields = {}) {
    const size_t n_cells = arity ? cells.size() / arity : 0;
    file << "    <Piece NumberOfPoints=\"" << points.size() << "\" NumberOfCells=\"" << n_cells << "\">\n"
         << "      <Points>\n"
         << "        <DataArray type=\"Float64\" NumberOfComponents=\"3\" format=\"ascii\">\n";
    for (const P3& p : points) file << "          " << p[0] << " " << p[1] << " " << p[2] << "\n";
    file << "        </DataArray>\n      </Points>\n";
    if (!fields.empty()) {
      file << "      <PointData";
      for (const PointField& f : fields)
        if (f.components == 1) {
          file << " Scalars=\"" << f.name << "\"";
          break;
        }
      for (const PointField& f : fields)
        if (f.components == 3) {
          file << " Vectors=\"" << f.name << "\"";
          break;
        }
      file << ">\n";
      for (const PointField& f : fields) {
        file << "        <DataArray type=\"Float64\" Name=\"" << f.name << "\"";
        if (f.components > 1) file << " NumberOfComponents=\"" << f.components << "\"";
        file << " format=\"ascii\">\n";
        for (size_t i = 0; i < points.size(); i++) {
          file << "         ";
          for (int c = 0; c < f.components; c++) {
            const size_t k = i * f.components + c;
            file << " " << (k < f.values.size() ? f.values[k] : 0.0);
          }
          file << "\n";
        }
        file << "        </DataArray>\n";
      }
      file << "      </PointData>\n";
    }
    if (!cell_fields.empty()) {
      file << "      <CellData>\n";
      for (const PointField& f : cell_fields) {
        file << "        <DataArray type=\"Float64\" Name=\"" << f.name << "\"";
        if (f.components > 1) file << " NumberOfComponents=\"" << f.components << "\"";
        file << " format=\"ascii\">\n";
        for (size_t i = 0; i < n_cells; i++) {
          file << "         ";
          for (int c = 0; c < f.components; c++) {
            const size_t k = i * f.components + c;
            file << " " << (k < f.values.size() ? f.values[k] : 0.0);
          }
          file << "\n";
        }
        file << "        </DataArray>\n";
      }
      file << "      </CellData>\n";
    }
    file << "      <Cells>\n        <DataArray type=\"Int32\" Name=\"connectivity\" format=\"ascii\">\n";
    for (size_t c = 0; c < n_cells; c++) {
      file << "         ";
      for (int k = 0; k < arity; k++) file << " " << cells[c * arity + k];
      file << "\n";
    }
    file << "        </DataArray>\n        <DataArray type=\"Int32\" Name=\"offsets\" format=\"ascii\">\n";
    for (size_t c = 0; c < n_cells; c++) file << "          " << (c + 1) * arity << "\n";
    file << "        </DataArray>\n        <DataArray type=\"UInt8\" Name=\"types\" format=\"ascii\">\n";
    for (size_t c = 0; c < n_cells; c++) file << "          " << vtk_type << "\n";
    file << "        </DataArray>\n      </Cells>\n    </Piece>\n";
  }

  // T10 mesh as linear tets on the four corner nodes + nodal scalar "pressure" (visualization_utils.h:491-589)
  static bool ExportMeshToVTU(const tlfea::MatrixXd& nodes, const tlfea::MatrixXi& elements,
                              const tlfea::VectorXd& scalarField, const std::string& filename) {
    std::vector<P3> pts(nodes.rows());
    PointField p{"pressure", 1, std::vector<double>(nodes.rows(), 0.0)};
    for (int i = 0; i < nodes.rows(); i++) {
      pts[i] = {nodes(i, 0), nodes(i, 1), nodes(i, 2)};
      if (i < scalarField.size()) p.values[i] = scalarField(i);
    }
    if (!WriteVTU(filename, pts, corner_tets(elements), 4, 10, {p})) return false;
    std::cout << "Exported mesh with " << nodes.rows() << " nodes and " << elements.rows() << " elements to " << filename
              << std::endl;
    return true;
  }

  // T10 mesh at `nodes` + nodal "displacement" vectors [dx0, dy0, dz0, dx1, ...] and their magnitude; entries past the
  // end of `displacement` read as zero (visualization_utils.h:718-846)
  static bool ExportMeshWithDisplacement(const tlfea::MatrixXd& nodes, const tlfea::MatrixXi& elements,
                                         const tlfea::VectorXd& displacement, const std::string& filename) {
    const int n = nodes.rows();
    std::vector<P3> pts(n);
    PointField d{"displacement", 3, std::vector<double>(3 * (size_t)n, 0.0)}, m{"displacement_magnitude", 1, std::vector<double>(n)};
    for (int i = 0; i < n; i++) {
      pts[i] = {nodes(i, 0), nodes(i, 1), nodes(i, 2)};
      double s = 0.0;
      for (int c = 0; c < 3; c++) {
        const double v = 3 * i + c < displacement.size() ? displacement(3 * i + c) : 0.0;
        d.values[3 * (size_t)i + c] = v;
        s += v * v;
      }
      m.values[i] = std::sqrt(s);
    }
    return WriteVTU(filename, pts, corner_tets(elements), 4, 10, {m, d});
  }

  // T10 mesh at `nodes` + nodal "displacement" (3), Cauchy "stress" (6: xx yy zz xy yz zx, N x 6) and "von_mises" (1),
  // as GPU_FEAT10_Data::RetrieveNodalStressToCPU returns them (no reference counterpart)
  static bool ExportMeshWithStress(const tlfea::MatrixXd& nodes, const tlfea::MatrixXi& elements,
                                   const tlfea::VectorXd& displacement, const tlfea::MatrixXd& nodal_sigma6,
                                   const tlfea::VectorXd& nodal_von_mises, const std::string& filename) {
    const int n = nodes.rows();
    std::vector<P3> pts(n);
    PointField d{"displacement", 3, std::vector<double>(3 * (size_t)n, 0.0)}, s{"stress", 6, std::vector<double>(6 * (size_t)n, 0.0)},
        m{"von_mises", 1, std::vector<double>(n, 0.0)};
    for (int i = 0; i < n; i++) {
      pts[i] = {nodes(i, 0), nodes(i, 1), nodes(i, 2)};
      for (int c = 0; c < 3; c++)
        if (3 * i + c < displacement.size()) d.values[3 * (size_t)i + c] = displacement(3 * i + c);
      if (i < nodal_sigma6.rows() && nodal_sigma6.cols() == 6)
        for (int c = 0; c < 6; c++) s.values[6 * (size_t)i + c] = nodal_sigma6(i, c);
      if (i < nodal_von_mises.size()) m.values[i] = nodal_von_mises(i);
    }
    return WriteVTU(filename, pts, corner_tets(elements), 4, 10, {m, d, s});
  }

  // T10 mesh at `nodes` + point data "stress" (6), "von_mises" (1) and "principal" (3: s1 s2 s3) of the recovered nodal
  // field and cell data "eta" (1: the element's ZZ error indicator eta_e), as GPU_FEAT10_Data::RetrieveRecoveredStressToCPU,
  // RetrievePrincipalStressToCPU (N x 4 values) and RetrieveErrorIndicatorToCPU (eta_e^2) return them (no reference
  // counterpart)
  static bool ExportMeshWithRecoveredStress(const tlfea::MatrixXd& nodes, const tlfea::MatrixXi& elements,
                                            const tlfea::MatrixXd& nodal_sigma6, const tlfea::VectorXd& nodal_von_mises,
                                            const tlfea::MatrixXd& nodal_principal, const tlfea::VectorXd& eta2,
                                            const std::string& filename) {
    const int n = nodes.rows(), E = elements.rows();
    if (nodal_sigma6.rows() != n || nodal_sigma6.cols() != 6 || nodal_von_mises.size() != n || nodal_principal.rows() != n ||
        nodal_principal.cols() < 3 || eta2.size() != E) {
      std::cerr << "ExportMeshWithRecoveredStress: N x 6 stresses, N von Mises values, N x 3 (or 4) principal values and E "
                   "indicator values expected" << std::endl;
      return false;
    }
    std::vector<P3> pts(n);
    PointField s{"stress", 6, std::vector<double>(6 * (size_t)n)}, m{"von_mises", 1, std::vector<double>(n)},
        p{"principal", 3, std::vector<double>(3 * (size_t)n)}, eta{"eta", 1, std::vector<double>(E)};
    for (int i = 0; i < n; i++) {
      pts[i] = {nodes(i, 0), nodes(i, 1), nodes(i, 2)};
      for (int c = 0; c < 6; c++) s.values[6 * (size_t)i + c] = nodal_sigma6(i, c);
      for (int c = 0; c < 3; c++) p.values[3 * (size_t)i + c] = nodal_principal(i, c);
      m.values[i] = nodal_von_mises(i);
    }
    for (int e = 0; e < E; e++) eta.values[e] = std::sqrt(std::max(0.0, eta2(e)));
    return WriteVTU(filename, std::vector<Piece>{Piece{pts, corner_tets(elements), 4, 10, {m, p, s}, {eta}}});
  }

  // One hexahedron per shell: the four corner positions (coefficient slot 0 of each node) pushed -/+ thickness/2 along
  // the element normal (p1-p0) x (p3-p0); bottom face first (visualization_utils.h:848-955)
  static bool ExportANCF3443ToVTU(const tlfea::VectorXd& x12, const tlfea::VectorXd& y12, const tlfea::VectorXd& z12,
                                  const tlfea::MatrixXi& element_connectivity, double thickness,
                                  const std::string& filename) {
    const int E = element_connectivity.rows();
    return WriteVTU(filename, shell_points(x12, y12, z12, element_connectivity, thickness), iota_cells(E, 8), 8, 12);
  }

  // One hexahedron per beam: a width x height rectangle at each end node, in the frame built from the chord tangent t,
  // n = t x ref (ref = z, or y when t is within ~26 degrees of z) and b = t x n (visualization_utils.h:974-1097)
  static bool ExportANCF3243ToVTU(const tlfea::VectorXd& x12, const tlfea::VectorXd& y12, const tlfea::VectorXd& z12,
                                  const tlfea::MatrixXi& element_connectivity, double width, double height,
                                  const std::string& filename) {
    const int E = element_connectivity.rows();
    return WriteVTU(filename, beam_points(x12, y12, z12, element_connectivity, width, height), iota_cells(E, 8), 8, 12);
  }

  // What ExportANCF3443ToVTU (connectivity of 4 columns; `width` unused) or ExportANCF3243ToVTU (2 columns) writes, with
  // point data "von_mises" (1) and "stress" (6: xx yy zz xy yz zx) as GPU_ANCF*_Data::RetrieveANCFNodalStressToCPU returns
  // them: the hexahedra's corners carry the values of their mesh node, and a second piece holds the mesh nodes themselves
  // (slot-0 positions, one vertex cell each) with the n_nodes tuples (no reference counterpart)
  static bool ExportANCFMeshWithStress(const tlfea::VectorXd& x12, const tlfea::VectorXd& y12, const tlfea::VectorXd& z12,
                                       const tlfea::MatrixXi& element_connectivity, double width, double height,
                                       const tlfea::MatrixXd& nodal_sigma6, const tlfea::VectorXd& nodal_von_mises,
                                       const std::string& filename) {
    const int E = element_connectivity.rows(), nn = element_connectivity.cols(), n_nodes = x12.size() / 4;
    if ((nn != 2 && nn != 4) || nodal_sigma6.rows() != n_nodes || nodal_sigma6.cols() != 6 || nodal_von_mises.size() != n_nodes) {
      std::cerr << "ExportANCFMeshWithStress: connectivity of 2 or 4 columns and n_nodes x 6 / n_nodes stresses expected" << std::endl;
      return false;
    }
    auto fields = [&](size_t n_points, auto node_of) {
      PointField m{"von_mises", 1, std::vector<double>(n_points)}, s{"stress", 6, std::vector<double>(6 * n_points)};
      for (size_t i = 0; i < n_points; i++) {
        const int n = node_of(i);
        m.values[i] = nodal_von_mises(n);
        for (int c = 0; c < 6; c++) s.values[6 * i + c] = nodal_sigma6(n, c);
      }
      return std::vector<PointField>{m, s};
    };
    Piece hexa{nn == 4 ? shell_points(x12, y12, z12, element_connectivity, height)
                       : beam_points(x12, y12, z12, element_connectivity, width, height),
               iota_cells(E, 8), 8, 12, {}};
    // corner i of element e: shells bottom face then top face over the 4 nodes, beams 4 corners per end node
    hexa.fields = fields(hexa.points.size(), [&](size_t i) {
      const int e = static_cast<int>(i / 8), k = static_cast<int>(i % 8);
      return element_connectivity(e, nn == 4 ? k % 4 : k / 4);
    });
    Piece nodes{std::vector<P3>(n_nodes), iota_cells(n_nodes, 1), 1, 1, {}};
    for (int n = 0; n < n_nodes; n++) nodes.points[n] = position(x12, y12, z12, n);
    nodes.fields = fields(n_nodes, [](size_t i) { return static_cast<int>(i); });
    return WriteVTU(filename, {hexa, nodes});
  }

  // Mode shapes of SyncedNewtonSolver::ModalAnalysis (no reference counterpart).  T10: the mesh at `nodes` with
  // one vector point field "mode_k" per mode (modes[k] = [3 n_nodes], M-normalised as returned) and the field data
  // "frequency_hz" [n_modes].
  static bool ExportModeShapesToVTU(const tlfea::MatrixXd& nodes, const tlfea::MatrixXi& elements,
                                    const std::vector<std::vector<double>>& modes, const std::vector<double>& freq_hz,
                                    const std::string& filename) {
    const int n = nodes.rows();
    if (modes.size() != freq_hz.size()) {
      std::cerr << "ExportModeShapesToVTU: one frequency per mode expected" << std::endl;
      return false;
    }
    Piece piece{std::vector<P3>(n), corner_tets(elements), 4, 10, {}};
    for (int i = 0; i < n; i++) piece.points[i] = {nodes(i, 0), nodes(i, 1), nodes(i, 2)};
    for (size_t k = 0; k < modes.size(); k++) {
      if (modes[k].size() != 3 * (size_t)n) {
        std::cerr << "ExportModeShapesToVTU: mode " << k << " does not hold 3 values per node" << std::endl;
        return false;
      }
      piece.fields.push_back(PointField{"mode_" + std::to_string(k), 3, modes[k]});
    }
    return WriteVTU(filename, {piece}, {PointField{"frequency_hz", 1, freq_hz}});
  }
  // ANCF kinds (connectivity of 2 columns: ANCF-3243 beams, 4: ANCF-3443 shells; `width` unused for shells): the hexahedra
  // of ExportANCF3243ToVTU / ExportANCF3443ToVTU, every corner carrying the position-coefficient part of its mesh node's
  // mode vector (modes[k] = [3 n_coef], coefficient 4 node), a second piece with the mesh nodes themselves, and the same
  // field data
  static bool ExportModeShapesToVTU(const tlfea::VectorXd& x12, const tlfea::VectorXd& y12, const tlfea::VectorXd& z12,
                                    const tlfea::MatrixXi& element_connectivity, double width, double height,
                                    const std::vector<std::vector<double>>& modes, const std::vector<double>& freq_hz,
                                    const std::string& filename) {
    const int E = element_connectivity.rows(), nn = element_connectivity.cols(), n_nodes = x12.size() / 4;
    if ((nn != 2 && nn != 4) || modes.size() != freq_hz.size()) {
      std::cerr << "ExportModeShapesToVTU: connectivity of 2 or 4 columns and one frequency per mode expected" << std::endl;
      return false;
    }
    for (const auto& m : modes)
      if (m.size() != 12 * (size_t)n_nodes) {
        std::cerr << "ExportModeShapesToVTU: a mode does not hold 3 values per coefficient" << std::endl;
        return false;
      }
    auto fields = [&](size_t n_points, auto node_of) {
      std::vector<PointField> out;
      for (size_t k = 0; k < modes.size(); k++) {
        PointField f{"mode_" + std::to_string(k), 3, std::vector<double>(3 * n_points)};
        for (size_t i = 0; i < n_points; i++)
          for (int c = 0; c < 3; c++) f.values[3 * i + c] = modes[k][12 * (size_t)node_of(i) + c];
        out.push_back(f);
      }
      return out;
    };
    Piece hexa{nn == 4 ? shell_points(x12, y12, z12, element_connectivity, height)
                       : beam_points(x12, y12, z12, element_connectivity, width, height),
               iota_cells(E, 8), 8, 12, {}};
    hexa.fields = fields(hexa.points.size(), [&](size_t i) {
      const int e = static_cast<int>(i / 8), k = static_cast<int>(i % 8);
      return element_connectivity(e, nn == 4 ? k % 4 : k / 4);
    });
    Piece pts{std::vector<P3>(n_nodes), iota_cells(n_nodes, 1), 1, 1, {}};
    for (int n = 0; n < n_nodes; n++) pts.points[n] = position(x12, y12, z12, n);
    pts.fields = fields(n_nodes, [](size_t i) { return static_cast<int>(i); });
    return WriteVTU(filename, {hexa, pts}, {PointField{"frequency_hz", 1, freq_hz}});
  }

  // The sample points of GPU_ANCF*_Data::RetrieveContactPointsToCPU (rows of x, y, z, gap, pressure) as vertex cells with
  // point data "gap" and "pressure"; in_contact_only keeps the rows of pressure > 0 (the footprint)
  static bool ExportContactPointsToVTU(const tlfea::MatrixXd& pts, const std::string& filename, bool in_contact_only = false) {
    if (pts.cols() != 5) {
      std::cerr << "ExportContactPointsToVTU: rows of x, y, z, gap, pressure expected" << std::endl;
      return false;
    }
    Piece piece{{}, {}, 1, 1, {}};
    PointField gap{"gap", 1, {}}, pressure{"pressure", 1, {}};
    for (int i = 0; i < pts.rows(); i++) {
      if (in_contact_only && !(pts(i, 4) > 0.0)) continue;
      piece.points.push_back({pts(i, 0), pts(i, 1), pts(i, 2)});
      gap.values.push_back(pts(i, 3));
      pressure.values.push_back(pts(i, 4));
    }
    piece.cells = iota_cells(static_cast<int>(piece.points.size()), 1);
    piece.fields = {gap, pressure};
    return WriteVTU(filename, {piece});
  }

 private:
  static std::vector<P3> shell_points(const tlfea::VectorXd& x12, const tlfea::VectorXd& y12, const tlfea::VectorXd& z12,
                                      const tlfea::MatrixXi& element_connectivity, double thickness) {
    const int E = element_connectivity.rows();
    std::vector<P3> pts;
    pts.reserve(8 * (size_t)E);
    for (int e = 0; e < E; e++) {
      P3 p[4];
      for (int k = 0; k < 4; k++) p[k] = position(x12, y12, z12, element_connectivity(e, k));
      P3 nrm = cross(sub(p[1], p[0]), sub(p[3], p[0]));
      if (!normalize(nrm)) nrm = {0.0, 0.0, 1.0};
      for (double side : {-0.5, 0.5})
        for (int k = 0; k < 4; k++) pts.push_back(axpy(side * thickness, nrm, p[k]));
    }
    return pts;
  }
  static std::vector<P3> beam_points(const tlfea::VectorXd& x12, const tlfea::VectorXd& y12, const tlfea::VectorXd& z12,
                                     const tlfea::MatrixXi& element_connectivity, double width, double height) {
    const int E = element_connectivity.rows();
    std::vector<P3> pts;
    pts.reserve(8 * (size_t)E);
    const double su[4] = {-0.5, 0.5, 0.5, -0.5}, sv[4] = {-0.5, -0.5, 0.5, 0.5};
    for (int e = 0; e < E; e++) {
      const P3 end[2] = {position(x12, y12, z12, element_connectivity(e, 0)),
                         position(x12, y12, z12, element_connectivity(e, 1))};
      P3 t = sub(end[1], end[0]);
      if (!normalize(t)) t = {1.0, 0.0, 0.0};
      const P3 ref = std::fabs(t[2]) > 0.9 ? P3{0.0, 1.0, 0.0} : P3{0.0, 0.0, 1.0};
      P3 n = cross(t, ref);
      if (!normalize(n)) n = {0.0, 1.0, 0.0};
      P3 b = cross(t, n);
      if (!normalize(b)) b = {0.0, 0.0, 1.0};
      for (int s = 0; s < 2; s++)
        for (int k = 0; k < 4; k++) pts.push_back(axpy(sv[k] * height, b, axpy(su[k] * width, n, end[s])));
    }
    return pts;
  }
  static P3 position(const tlfea::VectorXd& x, const tlfea::VectorXd& y, const tlfea::VectorXd& z, int node) {
    return {x(4 * node), y(4 * node), z(4 * node)};
  }
  static P3 sub(const P3& a, const P3& b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
  static P3 axpy(double s, const P3& d, const P3& p) { return {p[0] + s * d[0], p[1] + s * d[1], p[2] + s * d[2]}; }
  static P3 cross(const P3& a, const P3& b) {
    return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  }
  static bool normalize(P3& v) {
    const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (n < 1e-12) return false;
    for (double& c : v) c /= n;
    return true;
  }
  static std::vector<int> iota_cells(int n_cells, int arity) {
    std::vector<int> c((size_t)n_cells * arity);
    for (size_t i = 0; i < c.size(); i++) c[i] = static_cast<int>(i);
    return c;
  }
  static std::vector<int> corner_tets(const tlfea::MatrixXi& elements) {
    std::vector<int> c;
    c.reserve(4 * (size_t)elements.rows());
    for (int e = 0; e < elements.rows(); e++)
      for (int k = 0; k < 4; k++) c.push_back(elements(e, k));
    return c;
  }
};

}  // namespace ANCFCPUUtils
