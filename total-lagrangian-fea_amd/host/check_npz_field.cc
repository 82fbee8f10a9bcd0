// check_npz_field -- the C++ MeshManager's scalar-field loader on its own (no GPU): loads `--copies` copies of a
// TetGen T10 mesh, reads one .npz field into the first copy and prints the unified field, one value per line.
//   ./check_npz_field --mesh=tests/golden/meshes/sphere.1 --npz=tests/golden/meshes/sphere.1.uncompressed.npz
//                     [--key=p_vertex] [--copies=2]
// Exit status: 0 loaded, 2 the loader refused the file, 1 bad arguments or mesh.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "tlfea_facade.h"

int main(int argc, char** argv) {
  std::string mesh, npz, key = "p_vertex";
  int copies = 2;
  for (int i = 1; i < argc; i++) {
    const std::string a(argv[i]);
    if (a.rfind("--mesh=", 0) == 0) mesh = a.substr(7);
    else if (a.rfind("--npz=", 0) == 0) npz = a.substr(6);
    else if (a.rfind("--key=", 0) == 0) key = a.substr(6);
    else if (a.rfind("--copies=", 0) == 0) copies = std::atoi(a.c_str() + 9);
    else {
      std::cerr << "Unknown argument: " << a << std::endl;
      return 1;
    }
  }
  if (mesh.empty() || npz.empty() || copies < 1) {
    std::cerr << "usage: check_npz_field --mesh=PREFIX --npz=FILE [--key=NAME] [--copies=N]" << std::endl;
    return 1;
  }
  ANCFCPUUtils::MeshManager mm;
  for (int k = 0; k < copies; k++)
    if (mm.LoadMesh(mesh + ".node", mesh + ".ele") < 0) return 1;
  if (!mm.LoadScalarFieldFromNpz(0, npz, key)) return 2;
  const tlfea::VectorXd& f = mm.GetAllScalarFields();
  for (int i = 0; i < f.size(); i++) std::printf("%.17g\n", f(i));
  return 0;
}
