"""Per-element materials without a GPU: the exported symbols, the Python layer's refusals before any ABI call, and the
build of the host series-bar driver."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

tl = importlib.import_module("total-lagrangian-fea_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "total-lagrangian-fea_amd", "host")
NEW = ("tlfea_t10_set_element_materials", "tlfea_t10_clear_element_materials", "tlfea_t10_get_element_materials")


def test_symbols_exported():
    lib = tl.load_library()
    for name in NEW:
        assert name in tl.exported_symbols()
        assert hasattr(lib, name)


class _NoAbi:
    """Stands in for the library: any call through it is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the C-ABI")


def _data(E=4, N=20):
    d = tl.GPU_FEAT10_Data(E, N)   # never initialised: no device needed
    d._lib = _NoAbi()
    return d


@pytest.mark.parametrize("ids,mats,model,msg", [
    ([0, 0, 0], [tl.ElementMaterial(E=1e7, nu=0.3)], "svk", "3 ids for 4 elements"),
    ([0, 0, 0, 2], [tl.ElementMaterial(E=1e7, nu=0.3), {"E": 2e7, "nu": 0.3}], "svk", r"ids must lie in 0\.\.1"),
    ([0, -1, 0, 0], [tl.ElementMaterial(E=1e7, nu=0.3)], "svk", r"ids must lie in 0\.\.0"),
    ([0, 0, 0, 0], [], "svk", "needs 1..256 entries"),
    ([0, 0, 0, 0], [tl.ElementMaterial()] * 257, "svk", "needs 1..256 entries"),
    ([0, 0, 0, 0], [tl.ElementMaterial(E=1e7, nu=0.3)], "neo_hookean", "unknown model"),
    ([0.0, 0.5, 0, 0], [tl.ElementMaterial(E=1e7, nu=0.3)], "svk", "ids must be integers"),
])
def test_python_refusals(ids, mats, model, msg):
    with pytest.raises(ValueError, match=msg):
        _data().SetElementMaterials(ids, mats, model)


def test_material_entry_fields_match_abi():
    names = [f[0] for f in tl.binding.MaterialEntryC._fields_]
    assert names == ["E", "nu", "mu10", "mu01", "kappa", "rho0", "eta", "lamd"]
    import dataclasses
    assert [f.name for f in dataclasses.fields(tl.ElementMaterial)] == names


def test_mesh_manager_element_ids():
    mm = tl.MeshManager()
    assert np.array_equal(mm.GetAllElementMeshIds(), np.zeros(0, dtype=np.int32))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_host_driver_builds_with_hipcc(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib_dir = os.path.join(ROOT, "total-lagrangian-fea_amd")
    out = tmp_path / "test_two_material_bar"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", str(out),
                           os.path.join(HOST, "test_two_material_bar.cc"), "-L" + lib_dir, "-ltlfea_hip",
                           "-Wl,-rpath," + lib_dir])
    assert out.exists()
