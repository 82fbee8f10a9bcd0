"""Hydroelastic contact between tetrahedral meshes -- Python mirror of the reference's HydroelasticPatchCollisionSystem
(lib_src/collision/HydroelasticPatchCollisionSystem.h, CollisionSystemBase.h) over the tlfea_contact_* C-ABI.

Every contact step runs on the GPU (broadphase, narrowphase, forces: csrc/contact_kernels.hip); there is no CPU path.

Deviation from the reference: besides BindNodesDevicePtr (one [x..., y..., z...] device buffer), BindElementData binds a
GPU_FEAT10_Data directly -- this engine keeps x, y and z in separate allocations, which the context reads at every
step -- and ApplyToElementData writes f_ext = base + contact force into it on the device.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from .binding import ContactPatchC, check, dp, ip, load_library


@dataclass
class CollisionSystemInput:  # CollisionSystemBase.h
    d_nodes_xyz: int = 0      # device pointer [x..., y..., z...] or 0 (positions already bound)
    n_nodes: int = 0
    d_vel_xyz: int = 0        # device pointer to 3N interleaved velocities or 0
    dt: float = 0.0


@dataclass
class CollisionSystemParams:  # CollisionSystemBase.h
    damping: float = 0.0
    friction: float = 0.0


@dataclass
class ContactPatch:  # HydroelasticNarrowphase.cuh ContactPatch
    vertices: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    normal: np.ndarray = field(default_factory=lambda: np.zeros(3))
    centroid: np.ndarray = field(default_factory=lambda: np.zeros(3))
    area: float = 0.0
    g_A: float = 0.0
    g_B: float = 0.0
    p_equilibrium: float = 0.0
    tetA_idx: int = -1
    tetB_idx: int = -1
    isValid: bool = False
    validOrientation: bool = False

    @property
    def numVertices(self):
        return self.vertices.shape[0]


def _patch(c):
    n = c.count
    return ContactPatch(np.array([[c.vertices[i][k] for k in range(3)] for i in range(n)]).reshape(n, 3),
                        np.array(c.normal[:]), np.array(c.centroid[:]), c.area, c.g_A, c.g_B, c.p_equilibrium,
                        c.tetA, c.tetB, bool(c.isValid), bool(c.validOrientation))


class HydroelasticPatchCollisionSystem:
    """HydroelasticPatchCollisionSystem(mesh_manager, initial_nodes, elements, pressure, elementMeshIds,
    enable_self_collision).  elements: E x 10 (T10) or E x 4 node ids; pressure: one value per node; elementMeshIds:
    one mesh id per element (None: from mesh_manager, or all 0 without one).  initial_nodes is accepted for the
    reference's signature; positions come from the bound buffer at every step."""

    def __init__(self, mesh_manager, initial_nodes, elements, pressure, elementMeshIds=None,
                 enable_self_collision=False):
        self._lib = load_library()
        conn = np.ascontiguousarray(elements, dtype=np.int32)
        if conn.ndim != 2 or conn.shape[1] not in (4, 10):
            raise ValueError("elements must be E x 10 or E x 4")
        self.n_elem, npe = conn.shape
        press = np.ascontiguousarray(pressure, dtype=np.float64).reshape(-1)
        self.n_nodes = press.size
        if initial_nodes is not None and np.asarray(initial_nodes).shape[0] != self.n_nodes:
            raise ValueError("pressure needs one value per node")
        if elementMeshIds is None and mesh_manager is not None:
            elementMeshIds = [mesh_manager.GetMeshIdFromElement(e) for e in range(self.n_elem)]
        mesh = None if elementMeshIds is None else np.ascontiguousarray(elementMeshIds, dtype=np.int32)
        self._h = C.c_void_p()
        cm = np.ascontiguousarray(conn.T)  # column-major E x npe
        check(self._lib.tlfea_contact_create(self.n_nodes, self.n_elem, npe, ip(cm), dp(press), ip(mesh),
                                             int(bool(enable_self_collision)), C.byref(self._h)))
        self._pairs = np.zeros((0, 2), dtype=np.int32)
        self._patches = []

    def Destroy(self):
        if self._h:
            check(self._lib.tlfea_contact_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.Destroy()
        except Exception:
            pass

    def BindNodesDevicePtr(self, d_nodes_xyz, n_nodes):
        check(self._lib.tlfea_contact_bind_nodes(self._h, C.c_void_p(int(d_nodes_xyz)), int(n_nodes)))

    def BindElementData(self, data):
        """Documented deviation: positions from a GPU_FEAT10_Data's own x / y / z buffers, read at every step."""
        check(self._lib.tlfea_contact_bind_t10(self._h, data._h))

    def Step(self, inp=None, params=None):
        inp = inp or CollisionSystemInput()
        params = params or CollisionSystemParams()
        if inp.d_nodes_xyz:
            self.BindNodesDevicePtr(inp.d_nodes_xyz, inp.n_nodes or self.n_nodes)
        vel = C.c_void_p(int(inp.d_vel_xyz)) if inp.d_vel_xyz else None
        check(self._lib.tlfea_contact_step(self._h, vel, C.c_double(params.damping), C.c_double(params.friction)))

    def SetBaseForce(self, f):
        f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
        check(self._lib.tlfea_contact_set_base_force(self._h, dp(f), int(f.size)))

    def ApplyToElementData(self):
        """f_ext of the bound GPU_FEAT10_Data = base force + contact force, on the device."""
        check(self._lib.tlfea_contact_apply_to_t10(self._h))

    def GetExternalForcesDevicePtr(self):
        return self._lib.tlfea_contact_force_device_ptr(self._h)

    def GetNumContacts(self):
        n = C.c_int()
        check(self._lib.tlfea_contact_num_pairs(self._h, C.byref(n)))
        return n.value

    def GetNumPatches(self):
        n = C.c_int()
        check(self._lib.tlfea_contact_num_patches(self._h, C.byref(n)))
        return n.value

    def RetrieveResults(self):
        n = self.GetNumContacts()
        pairs = np.zeros((n, 2), dtype=np.int32)
        check(self._lib.tlfea_contact_retrieve_pairs(self._h, ip(pairs)))
        raw = (ContactPatchC * max(n, 1))()
        check(self._lib.tlfea_contact_retrieve_patches(self._h, raw))
        self._pairs = pairs
        self._patches = [_patch(raw[k]) for k in range(n)]
        return self._pairs, self._patches

    def GetPairs(self):
        return self._pairs

    def GetAllPatches(self):
        return self._patches

    def GetValidPatches(self):
        return [p for p in self._patches if p.isValid]

    def RetrieveForces(self):
        f = np.zeros(3 * self.n_nodes)
        check(self._lib.tlfea_contact_retrieve_force(self._h, dp(f)))
        return f
