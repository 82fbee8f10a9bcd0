// tlfea_mesh_manager.h -- ANCFCPUUtils::MeshManager of the reference (lib_utils/mesh_manager.h:67-235,
// mesh_manager.cc:180-220, 443-570): several TetGen T10 meshes behind one node / element numbering, the entry point
// the multi-body drivers use before GPU_FEAT10_Data::Setup.  Same member names and return conventions.  Kept as ONE
// unified node / element array plus a table of instances: a transform rewrites the instance's slice in place (the
// reference keeps per-mesh copies and rebuilds the union after every call).  Per-node scalar fields (the hydroelastic pressure of
// the contact subsystem) come from SetScalarField, a raw binary file or a stored .npz (LoadScalarFieldFromNpz).
// Included by tlfea_facade.h.
#pragma once
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iterator>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace ANCFCPUUtils {

using Matrix4d = tlfea::MatrixXd;  // 4 x 4 homogeneous transform, column-major like Eigen::Matrix4d

inline Matrix4d identity4() {
  Matrix4d T(4, 4);
  for (int i = 0; i < 4; i++) T(i, i) = 1.0;
  return T;
}
inline Matrix4d rotationX(double a) {  // mesh_manager.h:10-18
  Matrix4d R = identity4();
  R(1, 1) = std::cos(a); R(1, 2) = -std::sin(a);
  R(2, 1) = std::sin(a); R(2, 2) = std::cos(a);
  return R;
}
inline Matrix4d rotationY(double a) {  // :20-29
  Matrix4d R = identity4();
  R(0, 0) = std::cos(a); R(0, 2) = std::sin(a);
  R(2, 0) = -std::sin(a); R(2, 2) = std::cos(a);
  return R;
}
inline Matrix4d rotationZ(double a) {
  Matrix4d R = identity4();
  R(0, 0) = std::cos(a); R(0, 1) = -std::sin(a);
  R(1, 0) = std::sin(a); R(1, 1) = std::cos(a);
  return R;
}
inline Matrix4d translation(double dx, double dy, double dz) {  // :31-37
  Matrix4d T = identity4();
  T(0, 3) = dx; T(1, 3) = dy; T(2, 3) = dz;
  return T;
}
inline Matrix4d uniformScale(double s) {  // :39-45
  Matrix4d S = identity4();
  S(0, 0) = S(1, 1) = S(2, 2) = s;
  return S;
}

struct MeshInstance {  // mesh_manager.h:50-56
  int node_offset, element_offset, num_nodes, num_elements;
  std::string name;
};

// One array of a NumPy .npz: a walk over the ZIP local headers (stored entries only; ZIP64 sizes as numpy writes them)
// and the NPY v1 / v2 header ('descr', 'fortran_order', 'shape').  Plain C++, no zlib: a deflated entry
// (np.savez_compressed) is reported, as is a dtype other than the one asked for.
struct NpzArray {
  std::vector<double> f64;
  std::vector<long long> i64;

  // true when the archive holds an entry `key`.npy (whatever its dtype or compression)
  static bool Has(const std::string& path, const std::string& key) {
    NpzArray tmp;
    std::string err;
    return Read(path, key, "", &tmp, &err) || err.find("no array '" + key + "'") == std::string::npos;
  }

  static bool Read(const std::string& path, const std::string& key, const std::string& dtype, NpzArray* out,
                   std::string* err) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return fail(err, "cannot open " + path);
    std::vector<unsigned char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const std::string want = key + ".npy";
    size_t pos = 0;
    while (pos + 30 <= buf.size() && u32(buf, pos) == 0x04034b50u) {
      const unsigned flags = u16(buf, pos + 6), method = u16(buf, pos + 8);
      unsigned long long csize = u32(buf, pos + 18), usize = u32(buf, pos + 22);
      const size_t nlen = u16(buf, pos + 26), xlen = u16(buf, pos + 28);
      if (pos + 30 + nlen + xlen > buf.size()) break;
      const std::string name(buf.begin() + pos + 30, buf.begin() + pos + 30 + nlen);
      const size_t xend = pos + 30 + nlen + xlen;  // inside buf (checked above)
      for (size_t x = pos + 30 + nlen; x + 4 <= xend;) {  // ZIP64 extended information
        const unsigned id = u16(buf, x), len = u16(buf, x + 2);
        const size_t end = std::min(x + 4 + len, xend);
        if (id == 0x0001) {
          size_t q = x + 4;
          if (usize == 0xffffffffull && q + 8 <= end) usize = u64(buf, q), q += 8;
          if (csize == 0xffffffffull && q + 8 <= end) csize = u64(buf, q);
        }
        x += 4 + len;
      }
      if (flags & 8) return fail(err, path + ": entries with trailing data descriptors are not supported");
      const size_t data = pos + 30 + nlen + xlen;
      if (data + csize > buf.size()) break;
      if (name == want) {
        if (method != 0)
          return fail(err, path + ": '" + key + "' is compressed (np.savez_compressed); only stored .npz files are read");
        return parse_npy(buf, data, data + usize, dtype, path + ":" + key, out, err);
      }
      pos = data + csize;
    }
    return fail(err, path + ": no array '" + key + "'");
  }

 private:
  static bool fail(std::string* err, const std::string& m) {
    if (err) *err = m;
    return false;
  }
  static unsigned u16(const std::vector<unsigned char>& b, size_t p) { return b[p] | (b[p + 1] << 8); }
  static unsigned u32(const std::vector<unsigned char>& b, size_t p) { return u16(b, p) | (u16(b, p + 2) << 16); }
  static unsigned long long u64(const std::vector<unsigned char>& b, size_t p) {
    return u32(b, p) | (static_cast<unsigned long long>(u32(b, p + 4)) << 32);
  }
  static bool parse_npy(const std::vector<unsigned char>& b, size_t p, size_t end, const std::string& dtype,
                        const std::string& what, NpzArray* out, std::string* err) {
    if (end > b.size() || end < p + 10 || b[p] != 0x93 || std::string(b.begin() + p + 1, b.begin() + p + 6) != "NUMPY")
      return fail(err, what + ": not an NPY array");
    const int major = b[p + 6];
    size_t hlen, h0;
    if (major == 1) hlen = u16(b, p + 8), h0 = p + 10;
    else if (major == 2 || major == 3) hlen = u32(b, p + 8), h0 = p + 12;
    else return fail(err, what + ": NPY version " + std::to_string(major) + " is not supported");
    if (h0 + hlen > end) return fail(err, what + ": truncated NPY header");
    const std::string h(b.begin() + h0, b.begin() + h0 + hlen);
    const size_t d = h.find("'descr'");
    const size_t q1 = d == std::string::npos ? d : h.find('\'', d + 7);
    const size_t q2 = q1 == std::string::npos ? q1 : h.find('\'', q1 + 1);
    if (q2 == std::string::npos) return fail(err, what + ": NPY header without 'descr'");
    const std::string descr = h.substr(q1 + 1, q2 - q1 - 1);
    if (descr != dtype) return fail(err, what + ": dtype " + descr + ", expected " + dtype);
    if (h.find("'fortran_order': True") != std::string::npos) return fail(err, what + ": Fortran-ordered array");
    const size_t s = h.find("'shape'"), l = s == std::string::npos ? s : h.find('(', s), r = l == std::string::npos ? l : h.find(')', l);
    if (r == std::string::npos) return fail(err, what + ": NPY header without 'shape'");
    unsigned long long count = 1;
    std::string dims = h.substr(l + 1, r - l - 1);
    for (size_t k = 0; k < dims.size();) {
      while (k < dims.size() && !isdigit(static_cast<unsigned char>(dims[k]))) k++;
      if (k == dims.size()) break;
      unsigned long long v = 0;
      while (k < dims.size() && isdigit(static_cast<unsigned char>(dims[k]))) v = 10 * v + (dims[k++] - '0');
      count *= v;
    }
    const size_t data = h0 + hlen;
    if (data + 8 * count > end) return fail(err, what + ": NPY data shorter than its shape");
    out->f64.clear();
    out->i64.clear();
    for (unsigned long long k = 0; k < count; k++) {
      const unsigned long long bits = u64(b, data + 8 * k);
      if (dtype == "<f8") {
        double v;
        std::memcpy(&v, &bits, 8);
        out->f64.push_back(v);
      } else {
        out->i64.push_back(static_cast<long long>(bits));
      }
    }
    return true;
  }
};

class MeshManager {
 public:
  MeshManager() { Clear(); }

  // -> instance id, -1 when either file cannot be read (mesh_manager.cc:180-220)
  int LoadMesh(const std::string& node_file, const std::string& elem_file, const std::string& name = "") {
    tlfea::MatrixXd nodes;
    tlfea::MatrixXi elems;
    const int nn = FEAT10_read_nodes(node_file, nodes);
    const int ne = FEAT10_read_elements(elem_file, elems);
    if (nn <= 0 || ne <= 0) {
      std::cerr << "MeshManager: Failed to load mesh from " << node_file << " and " << elem_file << std::endl;
      return -1;
    }
    const int id = GetNumMeshes();
    const int n0 = GetTotalNodes(), e0 = GetTotalElements();
    inst_.push_back({n0, e0, nn, ne, name.empty() ? "mesh_" + std::to_string(id) : name});
    tlfea::MatrixXd all(n0 + nn, 3);
    for (int c = 0; c < 3; c++) {
      for (int i = 0; i < n0; i++) all(i, c) = nodes_(i, c);
      for (int i = 0; i < nn; i++) all(n0 + i, c) = nodes(i, c);
    }
    const int cols = e0 ? elems_.cols() : elems.cols();
    tlfea::MatrixXi alle(e0 + ne, cols);
    for (int c = 0; c < cols; c++) {
      for (int e = 0; e < e0; e++) alle(e, c) = elems_(e, c);
      for (int e = 0; e < ne; e++) alle(e0 + e, c) = elems(e, c) + n0;  // shift into the unified numbering
    }
    nodes_ = all;
    elems_ = alle;
    if (has_fields_) {  // a mesh loaded after fields were set contributes zeros until its own field arrives
      tlfea::VectorXd f(n0 + nn);
      for (int i = 0; i < n0; i++) f(i) = fields_(i);
      fields_ = f;
    }
    field_set_.push_back(false);
    return id;
  }

  void TransformMesh(int mesh_id, const Matrix4d& T) {  // mesh_manager.cc:467-482
    if (mesh_id < 0 || mesh_id >= GetNumMeshes()) {
      std::cerr << "MeshManager: Invalid mesh_id " << mesh_id << std::endl;
      return;
    }
    const MeshInstance& m = inst_[mesh_id];
    for (int i = m.node_offset; i < m.node_offset + m.num_nodes; i++) {
      const double p[3] = {nodes_(i, 0), nodes_(i, 1), nodes_(i, 2)};
      for (int r = 0; r < 3; r++) nodes_(i, r) = T(r, 0) * p[0] + T(r, 1) * p[1] + T(r, 2) * p[2] + T(r, 3);
    }
  }
  void TranslateMesh(int mesh_id, double dx, double dy, double dz) { TransformMesh(mesh_id, translation(dx, dy, dz)); }

  const tlfea::MatrixXd& GetAllNodes() const { return nodes_; }
  const tlfea::MatrixXi& GetAllElements() const { return elems_; }
  const MeshInstance& GetMeshInstance(int mesh_id) const {  // mesh_manager.cc:527-533
    if (mesh_id < 0 || mesh_id >= GetNumMeshes())
      throw std::out_of_range("MeshManager: Invalid mesh_id " + std::to_string(mesh_id));
    return inst_[mesh_id];
  }
  int GetNumMeshes() const { return static_cast<int>(inst_.size()); }
  int GetTotalNodes() const { return inst_.empty() ? 0 : inst_.back().node_offset + inst_.back().num_nodes; }
  int GetTotalElements() const { return inst_.empty() ? 0 : inst_.back().element_offset + inst_.back().num_elements; }

  // mesh_manager.cc LoadScalarFieldFromNpz: a field shorter than the mesh (values on the vertices of a T10 mesh) is
  // scattered through `original_vertex_ids` (1-based when 0 is absent and the smallest id is 1), all other nodes 0;
  // otherwise the field maps node by node, and a field longer than the mesh is refused.  Stored (uncompressed) .npz
  // only, float64 values and int64 ids (NpzArray below).
  bool LoadScalarFieldFromNpz(int mesh_id, const std::string& npz_file, const std::string& field_key = "p_vertex") {
    if (mesh_id < 0 || mesh_id >= GetNumMeshes()) {
      std::cerr << "MeshManager: Invalid mesh_id " << mesh_id << std::endl;
      return false;
    }
    const int n = inst_[mesh_id].num_nodes;
    NpzArray vals, ids;
    std::string err;
    if (!NpzArray::Read(npz_file, field_key, "<f8", &vals, &err)) {
      std::cerr << "MeshManager: " << err << std::endl;
      return false;
    }
    bool have_ids = false;
    if (NpzArray::Has(npz_file, "original_vertex_ids")) {
      if (!NpzArray::Read(npz_file, "original_vertex_ids", "<i8", &ids, &err)) {
        std::cerr << "MeshManager: " << err << std::endl;
        return false;
      }
      have_ids = true;
    }
    const long long nv = static_cast<long long>(vals.f64.size());
    if (nv > n) {
      std::cerr << "MeshManager: field '" << field_key << "' has " << nv << " values, mesh " << mesh_id << " has " << n
                << " nodes" << std::endl;
      return false;
    }
    tlfea::VectorXd field(n);
    for (int i = 0; i < n; i++) field(i) = 0.0;
    if (nv < n && have_ids) {
      if (static_cast<long long>(ids.i64.size()) != nv) {
        std::cerr << "MeshManager: " << ids.i64.size() << " original_vertex_ids for " << nv << " values" << std::endl;
        return false;
      }
      long long lo = 0;
      bool has_zero = false;
      for (long long k = 0; k < nv; k++) {
        lo = k == 0 ? ids.i64[k] : std::min(lo, ids.i64[k]);
        has_zero = has_zero || ids.i64[k] == 0;
      }
      const long long shift = (nv > 0 && lo == 1 && !has_zero) ? 1 : 0;
      for (long long k = 0; k < nv; k++) {
        const long long id = ids.i64[k] - shift;
        if (id < 0 || id >= n) {
          std::cerr << "MeshManager: original_vertex_ids entry " << ids.i64[k] << " outside mesh " << mesh_id << std::endl;
          return false;
        }
        field(static_cast<int>(id)) = vals.f64[k];
      }
    } else {
      for (long long k = 0; k < nv; k++) field(static_cast<int>(k)) = vals.f64[k];
    }
    return SetScalarField(mesh_id, field);
  }
  bool LoadScalarFieldFromBinary(int mesh_id, const std::string& bin_file, int n_values) {  // raw float64 array
    std::ifstream f(bin_file, std::ios::binary);
    if (!f) {
      std::cerr << "MeshManager: Failed to open binary file " << bin_file << std::endl;
      return false;
    }
    tlfea::VectorXd v(n_values);
    f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(n_values) * sizeof(double));
    if (f.gcount() != static_cast<std::streamsize>(n_values) * static_cast<std::streamsize>(sizeof(double))) {
      std::cerr << "MeshManager: Failed to read " << n_values << " values from " << bin_file << std::endl;
      return false;
    }
    return SetScalarField(mesh_id, v);
  }
  bool SetScalarField(int mesh_id, const tlfea::VectorXd& field) {  // mesh_manager.cc:422-441
    if (mesh_id < 0 || mesh_id >= GetNumMeshes()) {
      std::cerr << "MeshManager: Invalid mesh_id " << mesh_id << std::endl;
      return false;
    }
    const MeshInstance& m = inst_[mesh_id];
    if (field.size() != m.num_nodes) {
      std::cerr << "MeshManager: Scalar field size (" << field.size() << ") does not match mesh node count ("
                << m.num_nodes << ")" << std::endl;
      return false;
    }
    if (!has_fields_) {
      fields_.resize(GetTotalNodes());
      has_fields_ = true;
    }
    for (int i = 0; i < m.num_nodes; i++) fields_(m.node_offset + i) = field(i);
    field_set_[mesh_id] = true;
    return true;
  }
  const tlfea::VectorXd& GetAllScalarFields() const { return fields_; }
  bool HasScalarFields() const { return has_fields_; }

  int GetMeshIdFromElement(int global_elem_idx) const {
    for (int k = 0; k < GetNumMeshes(); k++)
      if (global_elem_idx >= inst_[k].element_offset && global_elem_idx < inst_[k].element_offset + inst_[k].num_elements)
        return k;
    return -1;
  }
  // mesh instance of every element of GetAllElements() (the id table of GPU_FEAT10_Data::SetElementMaterials)
  std::vector<int> GetAllElementMeshIds() const {
    std::vector<int> ids;
    ids.reserve(GetTotalElements());
    for (int k = 0; k < GetNumMeshes(); k++) ids.insert(ids.end(), inst_[k].num_elements, k);
    return ids;
  }
  int GetMeshIdFromNode(int global_node_idx) const {
    for (int k = 0; k < GetNumMeshes(); k++)
      if (global_node_idx >= inst_[k].node_offset && global_node_idx < inst_[k].node_offset + inst_[k].num_nodes) return k;
    return -1;
  }
  void Clear() {
    inst_.clear();
    field_set_.clear();
    nodes_.resize(0, 3);
    elems_.resize(0, 0);
    fields_.resize(0);
    has_fields_ = false;
  }

 private:
  std::vector<MeshInstance> inst_;
  std::vector<bool> field_set_;
  tlfea::MatrixXd nodes_;
  tlfea::MatrixXi elems_;
  tlfea::VectorXd fields_;
  bool has_fields_ = false;
};

}  // namespace ANCFCPUUtils
