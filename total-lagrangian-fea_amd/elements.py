"""GPU_FEAT10_Data -- host mirror of the reference class (lib_src/elements/FEAT10Data.cuh:19-852) on the
C-ABI.  Method names, argument order and call-order contract follow the reference; Eigen vectors become
NumPy arrays, Eigen::MatrixXi connectivity is an (E,10) int array (sent column-major as the reference does)."""
import collections
import ctypes as C
import dataclasses

import numpy as np

from .binding import MaterialEntryC, ObstacleC, SurfaceLoadC, T10SurfaceLoadC, check, dp, ip, load_library
from .loads import MAX_LOADS, BoundaryFaces, FaceLoad, FollowerPressure, SurfaceTraction, _SurfaceLoad
from .obstacles import MAX_OBSTACLES, RigidField, as_c, fields_as_c

MAX_MATERIALS = 256  # table entries per object (include/tlfea_c.h)
_MODELS = {"svk": 0, "mooney_rivlin": 1, "mr": 1}


@dataclasses.dataclass
class ElementMaterial:
    """One entry of a per-element material table: E, nu (SVK) or mu10, mu01, kappa (Mooney-Rivlin), the density rho0
    and the Kelvin-Voigt damping eta, lamd.  Fields of the other model are ignored."""
    E: float = 0.0
    nu: float = 0.0
    mu10: float = 0.0
    mu01: float = 0.0
    kappa: float = 0.0
    rho0: float = 0.0
    eta: float = 0.0
    lamd: float = 0.0


ElementStress = collections.namedtuple("ElementStress", "sigma von_mises psi J volume")
NodalStress = collections.namedtuple("NodalStress", "sigma von_mises")
Energies = collections.namedtuple("Energies", "strain kinetic viscous_power reference_volume current_volume")
PrincipalStress = collections.namedtuple(
    "PrincipalStress", "nodal_values nodal_tau_max nodal_directions element_values element_tau_max element_directions")
ErrorEstimate = collections.namedtuple("ErrorEstimate", "eta2 n2 eta_rel clamped")


def size_factors(eta2, n2, target_rel):
    """Element size factors for a target relative error from the retrieved indicator arrays (numpy only):
    clip(sqrt(target_rel sqrt((n^2 + eta^2) / E) / eta_e), 0.25, 4), the totals summed in element order."""
    eta2, n2 = np.asarray(eta2, dtype=np.float64), np.asarray(n2, dtype=np.float64)
    allowed = target_rel * np.sqrt((n2.sum() + eta2.sum()) / eta2.size)   # the error every element may carry
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.sqrt(allowed / np.sqrt(eta2))
    return np.clip(np.where(np.isnan(f), 4.0, f), 0.25, 4.0)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class GPU_FEAT10_Data:
    TYPE = "TYPE_T10"  # ElementBase.h:20
    S, Q = 10, 5       # shape functions / force quadrature points per element

    def __init__(self, num_elements, num_nodes):
        self._lib = load_library()
        self.n_elem, self.n_coef = int(num_elements), int(num_nodes)
        self._h = C.c_void_p()
        self._initialized = False

    # -- lifecycle ------------------------------------------------------------------------------
    def Initialize(self):
        check(self._lib.tlfea_t10_create(self.n_elem, self.n_coef, C.byref(self._h)))
        self._initialized = True

    def Destroy(self):
        if self._initialized:
            check(self._lib.tlfea_t10_destroy(self._h))
            self._initialized = False

    def Setup(self, tet5pt_x, tet5pt_y, tet5pt_z, tet5pt_weights, h_x12, h_y12, h_z12, element_connectivity):
        conn = np.asarray(element_connectivity)
        assert conn.shape == (self.n_elem, 10)
        conn_cm = np.ascontiguousarray(conn.T, dtype=np.int32)  # [10][E] == column-major E x 10
        qx, qy, qz, qw = _f64(tet5pt_x), _f64(tet5pt_y), _f64(tet5pt_z), _f64(tet5pt_weights)
        x, y, z = _f64(h_x12), _f64(h_y12), _f64(h_z12)
        assert x.size == y.size == z.size == self.n_coef
        check(self._lib.tlfea_t10_setup(self._h, dp(qx), dp(qy), dp(qz), dp(qw), dp(x), dp(y), dp(z), ip(conn_cm)))
        self._X0 = np.stack([x, y, z], axis=1)                    # reference geometry of GetBoundaryFaces

    # -- setters --------------------------------------------------------------------------------
    def SetDensity(self, rho0):
        check(self._lib.tlfea_t10_set_density(self._h, C.c_double(rho0)))

    def SetDamping(self, eta_damp, lambda_damp):
        check(self._lib.tlfea_t10_set_damping(self._h, C.c_double(eta_damp), C.c_double(lambda_damp)))

    def SetSVK(self, E=None, nu=None):
        if E is None:
            check(self._lib.tlfea_t10_set_svk_select(self._h))
        else:
            check(self._lib.tlfea_t10_set_svk(self._h, C.c_double(E), C.c_double(nu)))

    def SetMooneyRivlin(self, mu10, mu01, kappa):
        check(self._lib.tlfea_t10_set_mooney_rivlin(self._h, C.c_double(mu10), C.c_double(mu01), C.c_double(kappa)))

    def SetElementMaterials(self, ids, materials, model="svk"):
        """Per-element materials: ids[e] indexes `materials` (ElementMaterial or dicts of its fields); `model` ("svk" or
        "mooney_rivlin") applies to every entry.  Densities take effect at the next CalcMassMatrix.  While a table is
        set, SetSVK / SetMooneyRivlin / SetDensity / SetDamping fail; ClearElementMaterials returns to them."""
        if model not in _MODELS:
            raise ValueError(f"SetElementMaterials: unknown model {model!r} (one of {sorted(_MODELS)})")
        mats = [m if isinstance(m, ElementMaterial) else ElementMaterial(**m) for m in materials]
        if not 1 <= len(mats) <= MAX_MATERIALS:
            raise ValueError(f"SetElementMaterials: the table needs 1..{MAX_MATERIALS} entries, got {len(mats)}")
        eid = np.asarray(ids)
        if eid.ndim != 1 or eid.size != self.n_elem:
            raise ValueError(f"SetElementMaterials: {eid.size} ids for {self.n_elem} elements")
        if eid.size and not np.issubdtype(eid.dtype, np.integer):
            raise ValueError("SetElementMaterials: ids must be integers")
        if eid.size and (eid.min() < 0 or eid.max() >= len(mats)):
            raise ValueError(f"SetElementMaterials: ids must lie in 0..{len(mats) - 1}")
        eid = np.ascontiguousarray(eid, dtype=np.int32)
        table = (MaterialEntryC * len(mats))(*[MaterialEntryC(*dataclasses.astuple(m)) for m in mats])
        check(self._lib.tlfea_t10_set_element_materials(self._h, _MODELS[model], len(mats), table, ip(eid), int(eid.size)))

    def ClearElementMaterials(self):
        check(self._lib.tlfea_t10_clear_element_materials(self._h))

    def GetElementMaterialIds(self):
        """The element ids of the table set, or None in uniform mode."""
        n = C.c_int()
        check(self._lib.tlfea_t10_get_element_materials(self._h, C.byref(n), None))
        if n.value == 0:
            return None
        ids = np.zeros(self.n_elem, dtype=np.int32)
        check(self._lib.tlfea_t10_get_element_materials(self._h, C.byref(n), ip(ids)))
        return ids

    # -- rigid obstacles ----------------------------------------------------------------------
    def SetRigidObstacles(self, obstacles):
        """Replace the obstacle list (RigidPlane / RigidSphere, at most 16; an empty list clears it)."""
        obstacles = list(obstacles)
        if len(obstacles) > MAX_OBSTACLES:
            raise ValueError(f"at most {MAX_OBSTACLES} obstacles per object, got {len(obstacles)}")
        arr = (ObstacleC * max(1, len(obstacles)))(*[as_c(o) for o in obstacles])
        check(self._lib.tlfea_t10_set_obstacles(self._h, arr, len(obstacles)))

    def UpdateRigidObstacle(self, k, obstacle):
        """Replace obstacle k (move it between steps)."""
        o = as_c(obstacle)
        check(self._lib.tlfea_t10_update_obstacle(self._h, int(k), C.byref(o)))

    def ClearRigidObstacles(self):
        check(self._lib.tlfea_t10_clear_obstacles(self._h))

    def GetObstacleForces(self):
        """Contact force on every node (3N, the layout of f_ext) at the last gradient evaluation."""
        f = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_t10_get_obstacle_forces(self._h, dp(f)))
        return f

    def GetObstacleResultant(self, k):
        """(force of obstacle k on the mesh as a 3-vector, number of nodes in contact) at the last gradient evaluation."""
        out = np.zeros(4)
        check(self._lib.tlfea_t10_get_obstacle_resultant(self._h, int(k), dp(out)))
        return out[:3].copy(), int(round(out[3]))

    # -- field obstacles (DESIGN 3e''): any data class, beside the analytic list ----------------------------------------
    def SetFieldObstacles(self, fields):
        """Replace the list of field obstacles (RigidField; an empty list clears it).  Analytic and field obstacles
        together number at most 16; the analytic list stays as it is.  ANCF: after CalcDsDuPre."""
        arr, ptrs, n = fields_as_c(fields)
        check(self._lib.tlfea_set_field_obstacles(self._h, arr, ptrs, n))

    def UpdateFieldObstacle(self, k, field):
        """Move field k between steps: pose, velocity, stiffness, friction and eps_v of `field` (RigidField.moved); its grid
        must be the stored one, and the samples on the device are kept."""
        if not isinstance(field, RigidField):
            raise ValueError(f"expected a RigidField, got {type(field).__name__}")
        o = field.to_c()
        check(self._lib.tlfea_update_field_obstacle(self._h, int(k), C.byref(o)))

    def ClearFieldObstacles(self):
        check(self._lib.tlfea_clear_field_obstacles(self._h))

    def GetFieldObstacleResultant(self, k):
        """(force of field k on the mesh as a 3-vector, nodes or sample points in contact) at the last gradient evaluation."""
        out = np.zeros(4)
        check(self._lib.tlfea_get_field_obstacle_resultant(self._h, int(k), dp(out)))
        return out[:3].copy(), int(round(out[3]))

    def GetBoundaryTriangles(self, current=False):
        """The boundary of the mesh as a closed triangle surface: every 6-node face of GetBoundaryFaces split into four
        triangles over its corner and mid-edge nodes.  Returns (V (n, 3), T (m, 3)) with compact vertex numbering, outward
        orientation; the coordinates are the ones handed to Setup, or the current ones."""
        bf = self.GetBoundaryFaces()
        X = np.stack(self.RetrievePositionToCPU(), axis=1) if current else self._X0
        f = bf.nodes                                              # corners 0 1 2, mid-edge nodes 01 12 02
        tri = np.concatenate([f[:, [0, 3, 5]], f[:, [3, 1, 4]], f[:, [5, 4, 2]], f[:, [3, 4, 5]]], axis=1).reshape(-1, 3)
        used, inv = np.unique(tri, return_inverse=True)
        return np.ascontiguousarray(X[used]), inv.reshape(-1, 3).astype(np.int32)

    def GetSurfaceWeights(self):
        """Surface area share of every node (N; 0 inside the mesh): the weights of the contact model."""
        w = np.zeros(self.n_coef)
        check(self._lib.tlfea_t10_get_surface_weights(self._h, dp(w)))
        return w

    # -- distributed loads: beside f_ext, not in it --------------------------------------------------
    def SetGravity(self, acceleration):
        """Body acceleration (3-vector): the load M a on the position coefficients, from the mass matrix on the device.
        After CalcMassMatrix; follows a later CalcMassMatrix.  A zero vector removes it."""
        a = _f64(acceleration)
        if a.shape != (3,) or not np.all(np.isfinite(a)):
            raise ValueError("SetGravity: the acceleration must be a finite 3-vector")
        check(self._lib.tlfea_set_body_acceleration(self._h, dp(a)))

    def ClearLoads(self):
        """Remove the body acceleration and every surface load."""
        check(self._lib.tlfea_clear_loads(self._h))
        self._face_loads = []

    # -- surface loads on the boundary faces of a T10 mesh (DESIGN 3h') ------------------------------------------------
    def _t10_only(self, what):
        if self.S != 10:
            raise ValueError(f"{what}: T10 objects only (an ANCF object takes AddSurfaceTraction / AddFollowerPressure)")

    def GetBoundaryFaces(self):
        """The faces that belong to one tet only, in ascending (element, local face) order: elem (F), local_face (F),
        nodes (F, 6: corners, then the mid-edge nodes 01 12 02, ordered so that the normal points out of the mesh), and of
        the corner triangle in the reference configuration centroid (F, 3), outward unit normal (F, 3) and area (F).
        Select faces with numpy, e.g. np.nonzero(bf.normal[:, 2] > 0.99)[0]."""
        self._t10_only("GetBoundaryFaces")
        n = C.c_int()
        check(self._lib.tlfea_t10_get_boundary_faces(self._h, C.byref(n), None, None, None))
        elem, lf = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        nodes = np.zeros((n.value, 6), dtype=np.int32)
        check(self._lib.tlfea_t10_get_boundary_faces(self._h, C.byref(n), ip(elem), ip(lf), ip(nodes)))
        X = self._X0                                              # the coordinates handed to Setup
        a, b, c = X[nodes[:, 0]], X[nodes[:, 1]], X[nodes[:, 2]]
        nrm = np.cross(b - a, c - a)
        ln = np.linalg.norm(nrm, axis=1)
        self._n_boundary_faces = int(n.value)
        return BoundaryFaces(elem, lf, nodes, (a + b + c) / 3.0, nrm / ln[:, None], 0.5 * ln)

    def _add_face_load(self, load):
        self._t10_only("a face load")
        loads = getattr(self, "_face_loads", [])
        if len(loads) + 1 > MAX_LOADS:
            raise ValueError(f"at most {MAX_LOADS} surface loads per object")
        if getattr(self, "_n_boundary_faces", None) is None:
            n = C.c_int()
            check(self._lib.tlfea_t10_get_boundary_faces(self._h, C.byref(n), None, None, None))
            self._n_boundary_faces = int(n.value)
        load.check_against(self._n_boundary_faces)
        pairs = [ld.to_c() for ld in loads + [load]]              # the index arrays stay alive in `pairs` during the call
        arr = (T10SurfaceLoadC * len(pairs))(*[p[0] for p in pairs])
        check(self._lib.tlfea_t10_set_surface_loads(self._h, arr, len(pairs)))
        self._face_loads = loads + [load]
        return len(self._face_loads) - 1

    def AddFaceTraction(self, faces, traction, scale=1.0):
        """Dead traction (3-vector, force per reference area, fixed direction) on the boundary faces `faces` (indices into
        GetBoundaryFaces); returns the load's index."""
        return self._add_face_load(FaceLoad(0, faces, traction, scale))

    def AddFacePressure(self, faces, pressure, scale=1.0):
        """Pressure that follows the deformed boundary faces `faces` (positive pushes against the outward normal);
        returns the load's index.  Its load stiffness is left out of the Hessian, so Newton converges linearly in it:
        allow more inner iterations."""
        return self._add_face_load(FaceLoad(1, faces, pressure, scale))

    def SetFaceLoadScale(self, k, scale):
        """Change the scale factor of face load k (ramps) without sending the load again."""
        self._t10_only("SetFaceLoadScale")
        loads = getattr(self, "_face_loads", [])
        if not 0 <= int(k) < len(loads):
            raise ValueError(f"SetFaceLoadScale: index {k} outside the {len(loads)} face loads set")
        if not np.isfinite(scale):
            raise ValueError("SetFaceLoadScale: the scale must be finite")
        check(self._lib.tlfea_t10_update_load_scale(self._h, int(k), C.c_double(scale)))
        loads[int(k)].scale = float(scale)

    def GetLoadForces(self):
        """The distributed load on every coefficient (3 n_coef, the layout of f_ext) at the last gradient evaluation."""
        f = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_get_load_forces(self._h, dp(f)))
        return f

    def GetLoadResultant(self):
        """Sum of the load over the position coefficients (3-vector) at the last gradient evaluation."""
        out = np.zeros(3)
        check(self._lib.tlfea_get_load_resultant(self._h, dp(out)))
        return out

    def SetExternalForce(self, h_f_ext):
        f = _f64(h_f_ext)
        check(self._lib.tlfea_t10_set_external_force(self._h, dp(f), int(f.size)))

    def SetNodalFixed(self, fixed_nodes):
        fx = np.ascontiguousarray(fixed_nodes, dtype=np.int32)
        check(self._lib.tlfea_t10_set_nodal_fixed(self._h, ip(fx), int(fx.size)))
        self.fixed_nodes = fx.copy()  # constraint 3 k + c is component c of node fixed_nodes[k]

    def SetLinearConstraintsCSR(self, j_offsets, j_columns, j_values, rhs):
        """General linear constraints c = J x - rhs (ANCF3243Data.cuh:810-940); columns = 3*coef + component."""
        off = np.ascontiguousarray(j_offsets, dtype=np.int32)
        col = np.ascontiguousarray(j_columns, dtype=np.int32)
        val, r = _f64(j_values), _f64(rhs)
        if off.size == 0 or off[0] != 0:
            raise ValueError("SetLinearConstraintsCSR: invalid offsets.")
        if r.size + 1 != off.size:
            raise ValueError("SetLinearConstraintsCSR: offsets/rhs size mismatch.")
        if col.size != val.size:
            raise ValueError("SetLinearConstraintsCSR: columns/values size mismatch.")
        if off[-1] != col.size:
            raise ValueError("SetLinearConstraintsCSR: offsets.back != nnz.")
        check(self._lib.tlfea_t10_set_linear_constraints_csr(self._h, int(r.size), ip(off), ip(col), dp(val), dp(r)))

    def UpdateLinearConstraintRHS(self, rhs):
        """New right-hand side of the CSR constraints, J and the sparsity stay (ANCF3443Data.cuh:977-997)."""
        r = _f64(rhs)
        check(self._lib.tlfea_t10_update_linear_constraint_rhs(self._h, dp(r), int(r.size)))

    def GetConstraintMode(self):
        return int(self._lib.tlfea_t10_get_constraint_mode(self._h))

    def UpdateNodalFixed(self, fixed_nodes):
        fx = np.ascontiguousarray(fixed_nodes, dtype=np.int32)
        check(self._lib.tlfea_t10_update_nodal_fixed(self._h, ip(fx), int(fx.size)))
        self.fixed_nodes = fx.copy()

    def UpdatePositions(self, h_x12, h_y12, h_z12):
        x, y, z = _f64(h_x12), _f64(h_y12), _f64(h_z12)
        check(self._lib.tlfea_t10_update_positions(self._h, dp(x), dp(y), dp(z), int(x.size)))

    def UpdateConstraintTargets(self, h_x12, h_y12, h_z12):
        x, y, z = _f64(h_x12), _f64(h_y12), _f64(h_z12)
        check(self._lib.tlfea_t10_update_constraint_targets(self._h, dp(x), dp(y), dp(z), int(x.size)))

    # -- computations -----------------------------------------------------------------------------
    def CalcDnDuPre(self):
        check(self._lib.tlfea_t10_calc_dndu_pre(self._h))

    def BuildMassCSRPattern(self):
        check(self._lib.tlfea_t10_build_mass_csr_pattern(self._h))

    def CalcMassMatrix(self):
        check(self._lib.tlfea_t10_calc_mass_matrix(self._h))

    def CalcConstraintData(self):
        check(self._lib.tlfea_t10_calc_constraint_data(self._h))

    def ConvertToCSR_ConstraintJac(self):
        check(self._lib.tlfea_t10_convert_to_csr_constraint_jac(self._h))

    def ConvertToCSR_ConstraintJacT(self):
        check(self._lib.tlfea_t10_convert_to_csr_constraint_jact(self._h))

    BuildConstraintJacobianCSR = ConvertToCSR_ConstraintJac
    BuildConstraintJacobianTransposeCSR = ConvertToCSR_ConstraintJacT

    def CalcP(self):
        check(self._lib.tlfea_t10_calc_p(self._h))

    def CalcInternalForce(self):
        check(self._lib.tlfea_t10_calc_internal_force(self._h))

    # -- stress and energy recovery --------------------------------------------------------------
    def _stress_velocity(self, velocity):
        """(device pointer, host array) of CalcStress's velocity: a solver object gives its device pointer."""
        if velocity is None:
            return None, None
        if hasattr(velocity, "GetVelocityGuessDevicePtr"):
            return velocity.GetVelocityGuessDevicePtr(), None
        v = _f64(velocity).reshape(-1)
        if v.size != 3 * self.n_coef:
            raise ValueError(f"CalcStress: the velocity needs {3 * self.n_coef} entries, got {v.size}")
        return None, v

    def CalcStress(self, velocity=None, points=False):
        """Cauchy stress, strain-energy density and energies at the current positions.  `velocity`: None, a solver (its
        device velocity is used) or a host array of 3N; it adds a damped material's viscous stress and gives the kinetic
        energy and the viscous power.  `points` also keeps the stresses of the five quadrature points."""
        ptr, host = self._stress_velocity(velocity)
        if host is not None:
            check(self._lib.tlfea_t10_calc_stress_host(self._h, dp(host), int(bool(points))))
        else:
            check(self._lib.tlfea_t10_calc_stress(self._h, C.c_void_p(ptr), int(bool(points))))

    def RetrievePointStressToCPU(self):
        """[E][5][6]: xx yy zz xy yz zx per quadrature point (CalcStress(points=True))."""
        s = np.zeros((self.n_elem, 5, 6))
        check(self._lib.tlfea_t10_retrieve_point_stress(self._h, dp(s)))
        return s

    def RetrieveElementStressToCPU(self):
        """Reference-volume-weighted element means: sigma [E][6], von Mises of it, psi, J, and the element volume."""
        E = self.n_elem
        s, vm, psi, J, vol = np.zeros((E, 6)), np.zeros(E), np.zeros(E), np.zeros(E), np.zeros(E)
        check(self._lib.tlfea_t10_retrieve_element_stress(self._h, dp(s), dp(vm), dp(psi), dp(J), dp(vol)))
        return ElementStress(s, vm, psi, J, vol)

    def RetrieveNodalStressToCPU(self):
        """Element-volume-weighted nodal stress [N][6] and the von Mises stress of that tensor [N]."""
        s, vm = np.zeros((self.n_coef, 6)), np.zeros(self.n_coef)
        check(self._lib.tlfea_t10_retrieve_nodal_stress(self._h, dp(s), dp(vm)))
        return NodalStress(s, vm)

    def GetEnergies(self):
        out = np.zeros(5)
        check(self._lib.tlfea_t10_get_energies(self._h, dp(out)))
        return Energies(*out.tolist())

    def GetNodalStressDevicePtr(self):
        return self._lib.tlfea_t10_nodal_stress_device_ptr(self._h)

    # -- recovered stress, principal stresses, ZZ error indicator (DESIGN 3f'') ----------------------------------
    def RecoverStress(self, principal=True, directions=False):
        """Extrapolated nodal stress, principal stresses and the ZZ error indicator from the point stresses of the last
        CalcStress(points=True).  `directions` also keeps the principal directions (and implies `principal`)."""
        check(self._lib.tlfea_t10_recover_stress(self._h, int(bool(principal)), int(bool(directions))))

    def RecoverStressFromPoints(self, points, principal=True, directions=False):
        """The same launches on point stresses [E][5][6] given by the caller (needs CalcDnDuPre, no CalcStress)."""
        p = _f64(points)
        if p.size != self.n_elem * 30:
            raise ValueError(f"RecoverStressFromPoints: the point stresses need {self.n_elem * 30} entries, got {p.size}")
        check(self._lib.tlfea_t10_recover_stress_from_points(self._h, dp(p), int(bool(principal)), int(bool(directions))))

    def RetrieveRecoveredStressToCPU(self):
        """Recovered nodal stress [N][6] and the von Mises stress of that tensor [N]."""
        s, vm = np.zeros((self.n_coef, 6)), np.zeros(self.n_coef)
        check(self._lib.tlfea_t10_retrieve_recovered_stress(self._h, dp(s), dp(vm)))
        return NodalStress(s, vm)

    def RetrievePrincipalStressToCPU(self, directions=False):
        """Principal stresses of the recovered nodal tensors and of the element mean tensors: values [.][3] descending,
        tau_max = (s1 - s3) / 2 and, with `directions`, the unit eigenvectors [.][3][3] as rows of a right-handed frame
        (else None)."""
        N, E = self.n_coef, self.n_elem
        vn, ve = np.zeros((N, 4)), np.zeros((E, 4))
        dn, de = (np.zeros((N, 3, 3)), np.zeros((E, 3, 3))) if directions else (None, None)
        check(self._lib.tlfea_t10_retrieve_principal_stress(self._h, dp(vn), dp(dn), dp(ve), dp(de)))
        return PrincipalStress(vn[:, :3].copy(), vn[:, 3].copy(), dn, ve[:, :3].copy(), ve[:, 3].copy(), de)

    def RetrieveErrorIndicatorToCPU(self):
        """(eta_e^2 [E], n_e^2 [E]) of the ZZ error indicator."""
        eta2, n2 = np.zeros(self.n_elem), np.zeros(self.n_elem)
        check(self._lib.tlfea_t10_retrieve_error_indicator(self._h, dp(eta2), dp(n2)))
        return eta2, n2

    def GetErrorEstimate(self):
        out = np.zeros(4)
        check(self._lib.tlfea_t10_get_error_estimate(self._h, dp(out)))
        return ErrorEstimate(out[0], out[1], out[2], int(out[3]))

    def size_factors(self, target_rel):
        """Element size factors [E] for a target relative error, from the retrieved indicator (module size_factors)."""
        return size_factors(*self.RetrieveErrorIndicatorToCPU(), target_rel)

    def GetRecoveredStressDevicePtr(self):
        return self._lib.tlfea_t10_recovered_stress_device_ptr(self._h)

    def TimeRecoveryKernels(self, reps=20):
        """-> mean ms of (element records, nodal gather, nodal gather straight from the point blocks, principal
        stresses, error indicator, totals) over `reps` back-to-back launches each."""
        out = np.zeros(6)
        check(self._lib.tlfea_t10_time_recovery_kernels(self._h, int(reps), dp(out)))
        return out

    # -- material sensitivities ------------------------------------------------------------------
    def MaterialSensitivityShape(self):
        """(n_mat, P + 1): entries of the material table (1 without one) and the slots of the model set now -- SVK
        (lambda, mu, rho0), Mooney-Rivlin (mu10, mu01, kappa, rho0)."""
        n_mat, slots = C.c_int(), C.c_int()
        check(self._lib.tlfea_t10_material_sensitivity_shape(self._h, C.byref(n_mat), C.byref(slots)))
        return n_mat.value, slots.value

    def MaterialSensitivity(self, w, u=None):
        """The element kernel of the adjoint step and its reduction alone, at the current positions: for an adjoint field
        w and an acceleration field u [3N or N x 3], per element -sum_q dV (dP/dtheta_p)(F) : grad w for every stiffness
        parameter and -sum_q dV (N w).(N u) for the density.  -> (per_element [E, P + 1], per_material [n_mat, P + 1])."""
        w = _f64(w).reshape(-1)
        u = None if u is None else _f64(u).reshape(-1)
        if w.size != 3 * self.n_coef or (u is not None and u.size != w.size):
            raise ValueError(f"MaterialSensitivity: w and u need {3 * self.n_coef} entries")
        n_mat, slots = self.MaterialSensitivityShape()
        pe, pm = np.zeros((self.n_elem, slots)), np.zeros((n_mat, slots))
        check(self._lib.tlfea_t10_material_sensitivity(self._h, dp(w), dp(u), dp(pe), dp(pm)))
        return pe, pm

    def TimeSensitivityKernels(self, reps=20):
        """-> mean ms of (element kernel, reduction) over `reps` back-to-back launches each."""
        out = np.zeros(2)
        check(self._lib.tlfea_t10_time_sensitivity_kernels(self._h, int(reps), dp(out)))
        return out

    # -- shape sensitivities and the reference geometry ----------------------------------------------
    def ShapeSensitivity(self, w, u=None):
        """The element kernel of the shape adjoint and its gather alone, at the current positions: for an adjoint field w
        and an acceleration field u [3N or N x 3] (None: no mass term) -> X_bar [N, 3], the cotangent of the reference
        coordinates of every node."""
        w = _f64(w).reshape(-1)
        u = None if u is None else _f64(u).reshape(-1)
        if w.size != 3 * self.n_coef or (u is not None and u.size != w.size):
            raise ValueError(f"ShapeSensitivity: w and u need {3 * self.n_coef} entries")
        out = np.zeros((self.n_coef, 3))
        check(self._lib.tlfea_t10_shape_sensitivity(self._h, dp(w), dp(u), dp(out)))
        return out

    def TimeShapeKernels(self, reps=20):
        """-> mean ms of (element kernel, gather) over `reps` back-to-back launches each."""
        out = np.zeros(2)
        check(self._lib.tlfea_t10_time_shape_kernels(self._h, int(reps), dp(out)))
        return out

    def SetReferencePositions(self, X):
        """A new reference geometry X [N, 3] for the same connectivity: grad N, det J and an assembled mass matrix follow,
        as do boundary-face geometry, traction vectors and obstacle surface weights.  Current positions, velocities,
        multipliers and targets are left alone.  An inverted element is refused and leaves the old geometry in place."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.shape != (self.n_coef, 3):
            raise ValueError(f"SetReferencePositions: X must be [{self.n_coef}, 3], got {X.shape}")
        x, y, z = (np.ascontiguousarray(X[:, c]) for c in range(3))
        check(self._lib.tlfea_t10_set_reference_positions(self._h, dp(x), dp(y), dp(z), int(self.n_coef)))
        self._X0 = X.copy()

    def TimeStressKernels(self, velocity=None, points=False, reps=20):
        """-> mean ms of (point and element kernel, nodal gather, totals) over `reps` back-to-back launches each."""
        ptr, host = self._stress_velocity(velocity)
        if host is not None:
            raise ValueError("TimeStressKernels: pass a solver or None")
        out = np.zeros(3)
        check(self._lib.tlfea_t10_time_stress_kernels(self._h, C.c_void_p(ptr), int(bool(points)), int(reps), dp(out)))
        return out

    # -- getters ----------------------------------------------------------------------------------
    def get_n_elem(self):
        return self.n_elem

    def get_n_beam(self):
        return self.n_elem

    def get_n_coef(self):
        return self.n_coef

    def get_n_constraint(self):
        return self._lib.tlfea_t10_get_n_constraint(self._h)

    def Get_Is_Constraint_Setup(self):
        return bool(self._lib.tlfea_t10_is_constraint_setup(self._h))

    def GetX12DevicePtr(self):
        return self._lib.tlfea_t10_x12_device_ptr(self._h)

    def GetY12DevicePtr(self):
        return self._lib.tlfea_t10_y12_device_ptr(self._h)

    def GetZ12DevicePtr(self):
        return self._lib.tlfea_t10_z12_device_ptr(self._h)

    def GetExternalForceDevicePtr(self):
        return self._lib.tlfea_t10_external_force_device_ptr(self._h)

    def Get_Constraint_Ptr(self):
        return self._lib.tlfea_t10_constraint_device_ptr(self._h)

    # -- retrieval (reference layouts) ----------------------------------------------------------------
    def RetrieveMassCSRToCPU(self):
        nnz = C.c_int()
        check(self._lib.tlfea_t10_mass_csr_nnz(self._h, C.byref(nnz)))
        off = np.zeros(self.n_coef + 1, dtype=np.int32)
        col = np.zeros(nnz.value, dtype=np.int32)
        val = np.zeros(nnz.value)
        check(self._lib.tlfea_t10_retrieve_mass_csr(self._h, ip(off), ip(col), dp(val)))
        return off, col, val

    def RetrieveInternalForceToCPU(self):
        f = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_t10_retrieve_internal_force(self._h, dp(f)))
        return f

    def RetrieveExternalForceToCPU(self):
        f = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_t10_retrieve_external_force(self._h, dp(f)))
        return f

    def RetrievePositionToCPU(self):
        x, y, z = (np.zeros(self.n_coef) for _ in range(3))
        check(self._lib.tlfea_t10_retrieve_position(self._h, dp(x), dp(y), dp(z)))
        return x, y, z

    def RetrievePFromFToCPU(self):
        """[E][5] 3x3 matrices; flat storage is column-major per matrix like the reference."""
        P = np.zeros((self.n_elem, self.Q, 9))
        check(self._lib.tlfea_t10_retrieve_p_from_f(self._h, dp(P)))
        return P.reshape(self.n_elem, self.Q, 3, 3).transpose(0, 1, 3, 2)

    def RetrieveDeformationGradientToCPU(self):
        F = np.zeros((self.n_elem, self.Q, 9))
        check(self._lib.tlfea_t10_retrieve_deformation_gradient(self._h, dp(F)))
        return F.reshape(self.n_elem, self.Q, 3, 3).transpose(0, 1, 3, 2)

    def RetrieveDnDuPreToCPU(self):
        """[E][Q] S x 3 matrices (shape function, direction)."""
        g = np.zeros((self.n_elem, self.Q, 3, self.S))
        check(self._lib.tlfea_t10_retrieve_dndu_pre(self._h, dp(g)))
        return g.transpose(0, 1, 3, 2)

    def RetrieveDetJToCPU(self):
        d = np.zeros((self.n_elem, self.Q))
        check(self._lib.tlfea_t10_retrieve_detj(self._h, dp(d)))
        return d

    def RetrieveConnectivityToCPU(self):
        c = np.zeros((self.S, self.n_elem), dtype=np.int32)  # coefficient ids (T10: node ids)
        check(self._lib.tlfea_t10_retrieve_connectivity(self._h, ip(c)))
        return np.ascontiguousarray(c.T)

    def RetrieveConstraintDataToCPU(self):
        c = np.zeros(self.get_n_constraint())
        check(self._lib.tlfea_t10_retrieve_constraint_data(self._h, dp(c)))
        return c

    def RetrieveConstraintJacobianCSRToCPU(self):
        nc, nnz = self.get_n_constraint(), int(self._lib.tlfea_t10_constraint_jac_nnz(self._h))
        off, col, val = np.zeros(nc + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
        check(self._lib.tlfea_t10_retrieve_constraint_jac_csr(self._h, ip(off), ip(col), dp(val)))
        return off, col, val

    def RetrieveConstraintJacobianTransposeCSRToCPU(self):
        nnz = int(self._lib.tlfea_t10_constraint_jac_nnz(self._h))
        off, col, val = np.zeros(3 * self.n_coef + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
        check(self._lib.tlfea_t10_retrieve_constraint_jact_csr(self._h, ip(off), ip(col), dp(val)))
        return off, col, val

    def WriteOutputVTK(self, filename):
        check(self._lib.tlfea_t10_write_output_vtk(self._h, str(filename).encode()))


class _GPU_ANCF_Data(GPU_FEAT10_Data):
    """Common host mirror of GPU_ANCF3243_Data / GPU_ANCF3443_Data (lib_src/elements/ANCF3243Data.cuh:33-1152,
    ANCF3443Data.cuh).  4 coefficient vectors per node (r, r_u, r_v, r_w): n_coef = 4 * n_nodes;
    SetNodalFixed takes COEFFICIENT indices (ANCF3243Data.cuh:778-808)."""
    KIND = 0
    NN = 0

    def __init__(self, num_nodes, num_elements):
        self._lib = load_library()
        self.n_nodes, self.n_elem = int(num_nodes), int(num_elements)
        self.n_beam = self.n_elem
        self.n_coef = 4 * self.n_nodes
        self._h = C.c_void_p()
        self._initialized = False

    def Initialize(self):
        check(self._lib.tlfea_ancf_create(self.KIND, self.n_nodes, self.n_elem, C.byref(self._h)))
        self._initialized = True

    def PrintDsDuPre(self):
        """Text dump of the reference gradients per (element, point) (ANCF3243Data.cu:326-360)."""
        g, dj = self.RetrieveDnDuPreToCPU(), self.RetrieveDetJToCPU()
        for e in range(self.n_elem):
            for q in range(self.Q):
                print(f"\n=== Elem {e} Quadrature Point {q} detJ_ref={dj[e, q]:g} ===")
                print("        dN/dx       dN/dy       dN/dz")
                for i in range(self.S):
                    print(f"Shape {i}: " + " ".join(f"{g[e, q, i, j]:10.6f}" for j in range(3)) + " ")

    def _setup(self, length, width, height, mass_rule, force_rule, h_x12, h_y12, h_z12, connectivity):
        E = self.n_elem
        L, W, H = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (E,))) for a in
                   (length, width, height))
        mr = [_f64(a) for a in mass_rule]
        fr = [_f64(a) for a in force_rule]
        nqm = np.array([len(mr[0]), len(mr[1]), len(mr[2])], dtype=np.int32)
        nq = np.array([len(fr[0]), len(fr[1]), len(fr[2])], dtype=np.int32)
        conn = np.ascontiguousarray(np.asarray(connectivity).reshape(E, self.NN), dtype=np.int32)
        x, y, z = _f64(h_x12), _f64(h_y12), _f64(h_z12)
        assert x.size == y.size == z.size == self.n_coef
        check(self._lib.tlfea_ancf_setup(self._h, dp(L), dp(W), dp(H), dp(mr[0]), dp(mr[1]), dp(mr[2]), dp(mr[3]),
                                         dp(mr[4]), dp(mr[5]), ip(nqm), dp(fr[0]), dp(fr[1]), dp(fr[2]), dp(fr[3]),
                                         dp(fr[4]), dp(fr[5]), ip(nq), dp(x), dp(y), dp(z), ip(conn), 0))
        self._X0 = np.stack([x, y, z], axis=1)                    # reference coefficients: the targets of fixed ones

    def CalcDsDuPre(self):
        check(self._lib.tlfea_ancf_calc_dsdu_pre(self._h))

    CalcDnDuPre = CalcDsDuPre
    RetrieveDsDuPreToCPU = GPU_FEAT10_Data.RetrieveDnDuPreToCPU

    def get_n_beam(self):
        return self.n_elem

    # -- stress and energy recovery (DESIGN 3f'); CalcStress / Retrieve*StressToCPU stay T10-only and keep refusing -------
    def _ancf_stress_velocity(self, vel):
        if vel is not None and not hasattr(vel, "GetVelocityGuessDevicePtr") and np.size(vel) != 3 * self.n_coef:
            raise ValueError(f"CalcElementStress: the velocity needs {3 * self.n_coef} entries, got {np.size(vel)}")
        return self._stress_velocity(vel)

    def CalcElementStress(self, vel=None, want_points=False):
        """Cauchy stress, strain-energy density and energies at the current coefficients.  `vel`: None, a solver (its
        device velocity is used) or a host array of 3 n_coef; it adds a damped material's viscous stress and gives the
        kinetic energy and the viscous power.  `want_points` also keeps the stresses of the Q force-quadrature points."""
        ptr, host = self._ancf_stress_velocity(vel)
        if host is not None:
            check(self._lib.tlfea_ancf_calc_stress_host(self._h, dp(host), int(bool(want_points))))
        else:
            check(self._lib.tlfea_ancf_calc_stress(self._h, C.c_void_p(ptr), int(bool(want_points))))

    def RetrieveANCFPointStressToCPU(self):
        """[E][Q][6]: xx yy zz xy yz zx per force-quadrature point (CalcElementStress(want_points=True))."""
        s = np.zeros((self.n_elem, self.Q, 6))
        check(self._lib.tlfea_ancf_retrieve_point_stress(self._h, dp(s)))
        return s

    def RetrieveANCFElementStressToCPU(self):
        """Reference-volume-weighted element means: sigma [E][6], von Mises of it, psi, J, and the element volume."""
        E = self.n_elem
        s, vm, psi, J, vol = np.zeros((E, 6)), np.zeros(E), np.zeros(E), np.zeros(E), np.zeros(E)
        check(self._lib.tlfea_ancf_retrieve_element_stress(self._h, dp(s), dp(vm), dp(psi), dp(J), dp(vol)))
        return ElementStress(s, vm, psi, J, vol)

    def RetrieveANCFNodalStressToCPU(self):
        """Element-volume-weighted stress of every MESH node [n_nodes][6] and the von Mises stress of that tensor."""
        s, vm = np.zeros((self.n_nodes, 6)), np.zeros(self.n_nodes)
        check(self._lib.tlfea_ancf_retrieve_nodal_stress(self._h, dp(s), dp(vm)))
        return NodalStress(s, vm)

    def GetANCFEnergies(self):
        out = np.zeros(5)
        check(self._lib.tlfea_ancf_get_energies(self._h, dp(out)))
        return Energies(*out.tolist())

    def GetANCFNodalStressDevicePtr(self):
        return self._lib.tlfea_ancf_nodal_stress_device_ptr(self._h)

    def TimeANCFStressKernels(self, vel=None, want_points=False, reps=20):
        """-> mean ms of (point and element kernel, mesh-node gather, totals) over `reps` back-to-back launches each."""
        ptr, host = self._ancf_stress_velocity(vel)
        if host is not None:
            raise ValueError("TimeANCFStressKernels: pass a solver or None")
        out = np.zeros(3)
        check(self._lib.tlfea_ancf_time_stress_kernels(self._h, C.c_void_p(ptr), int(bool(want_points)), int(reps), dp(out)))
        return out

    # -- material sensitivities (DESIGN 3j'); MaterialSensitivity stays T10-only and keeps refusing ---------------------
    def ANCFMaterialSensitivityShape(self):
        """(1, P + 1): the object's one material and the slots of the model set now -- SVK (lambda, mu, rho0),
        Mooney-Rivlin (mu10, mu01, kappa, rho0)."""
        n_mat, slots = C.c_int(), C.c_int()
        check(self._lib.tlfea_ancf_material_sensitivity_shape(self._h, C.byref(n_mat), C.byref(slots)))
        return n_mat.value, slots.value

    def ANCFMaterialSensitivity(self, w, u=None):
        """The element kernel of the ANCF adjoint step and the sums alone, at the current coefficients: for an adjoint
        field w [3 n_coef or n_coef x 3], per element -sum_q dV (dP/dtheta_p)(F) : grad w over the force rule's points for
        every stiffness parameter; the density slot is -(M w) . u / rho0 for an acceleration field u (None: 0), with the
        density the mass matrix was assembled with.  -> (per_element [E, P], per_material [1, P + 1])."""
        w = _f64(w).reshape(-1)
        u = None if u is None else _f64(u).reshape(-1)
        if w.size != 3 * self.n_coef or (u is not None and u.size != w.size):
            raise ValueError(f"ANCFMaterialSensitivity: w and u need {3 * self.n_coef} entries")
        n_mat, slots = self.ANCFMaterialSensitivityShape()
        pe, pm = np.zeros((self.n_elem, slots - 1)), np.zeros((n_mat, slots))
        check(self._lib.tlfea_ancf_material_sensitivity(self._h, dp(w), dp(u), dp(pe), dp(pm)))
        return pe, pm

    def TimeANCFSensitivityKernels(self, reps=20):
        """-> mean ms of (element kernel, sums of its P planes) over `reps` back-to-back launches each."""
        out = np.zeros(2)
        check(self._lib.tlfea_ancf_time_sensitivity_kernels(self._h, int(reps), dp(out)))
        return out

    # -- surface loads: dead traction and follower pressure on element faces -------------------------------
    def _send_loads(self, loads):
        pairs = [ld.to_c() for ld in loads]                       # the index arrays stay alive in `pairs` during the call
        arr = (SurfaceLoadC * max(1, len(pairs)))(*[p[0] for p in pairs])
        check(self._lib.tlfea_ancf_set_surface_loads(self._h, arr, len(pairs)))

    def AddSurfaceLoad(self, load):
        """Append a SurfaceTraction / FollowerPressure to the object's list (at most 16); returns its index.  After Setup
        and CalcDsDuPre."""
        if not isinstance(load, _SurfaceLoad):
            raise ValueError(f"expected a SurfaceTraction or FollowerPressure, got {type(load).__name__}")
        loads = getattr(self, "_loads", [])
        if len(loads) + 1 > MAX_LOADS:
            raise ValueError(f"at most {MAX_LOADS} surface loads per object")
        load.check_against(self.S, self.n_elem)
        self._send_loads(loads + [load])
        self._loads = loads + [load]
        return len(self._loads) - 1

    def AddSurfaceTraction(self, face, elements, traction, scale=1.0):
        """Dead traction (force per reference area, fixed direction) on one face of `elements`; returns the load's index."""
        return self.AddSurfaceLoad(SurfaceTraction(face, elements, traction, scale))

    def AddFollowerPressure(self, face, elements, pressure, scale=1.0):
        """Pressure that follows the deformed face (positive pushes against its outward normal); returns the load's index.
        Its load stiffness is left out of the Hessian, so Newton converges linearly in it: allow more inner iterations."""
        return self.AddSurfaceLoad(FollowerPressure(face, elements, pressure, scale))

    def SetLoadScale(self, k, scale):
        """Change the scale factor of surface load k (ramps) without sending the load again."""
        loads = getattr(self, "_loads", [])
        if not 0 <= int(k) < len(loads):
            raise ValueError(f"SetLoadScale: index {k} outside the {len(loads)} surface loads set")
        if not np.isfinite(scale):
            raise ValueError("SetLoadScale: the scale must be finite")
        check(self._lib.tlfea_ancf_update_load_scale(self._h, int(k), C.c_double(scale)))
        loads[int(k)].scale = float(scale)

    def ClearLoads(self):
        """Remove every surface load and the body acceleration."""
        check(self._lib.tlfea_clear_loads(self._h))
        self._loads = []

    def GetLoadForces(self):
        """The distributed load on every coefficient (3 n_coef, the layout of f_ext) at the last gradient evaluation."""
        return super().GetLoadForces()

    def GetLoadResultant(self):
        """Sum of the load over the position coefficients 4 n (3-vector) at the last gradient evaluation."""
        return super().GetLoadResultant()

    # -- rigid obstacles (DESIGN 3e'): contact at 32 sample points per element ------------------------------------------
    POINTS = 32

    def SetRigidObstacles(self, obstacles):
        """Replace the obstacle list (RigidPlane / RigidSphere, at most 16; an empty list clears it).  After Setup and
        CalcDsDuPre."""
        obstacles = list(obstacles)
        if len(obstacles) > MAX_OBSTACLES:
            raise ValueError(f"at most {MAX_OBSTACLES} obstacles per object, got {len(obstacles)}")
        arr = (ObstacleC * max(1, len(obstacles)))(*[as_c(o) for o in obstacles])
        check(self._lib.tlfea_ancf_set_obstacles(self._h, arr, len(obstacles)))

    def UpdateRigidObstacle(self, k, obstacle):
        """Replace obstacle k (move it between steps)."""
        o = as_c(obstacle)
        check(self._lib.tlfea_ancf_update_obstacle(self._h, int(k), C.byref(o)))

    def ClearRigidObstacles(self):
        check(self._lib.tlfea_ancf_clear_obstacles(self._h))

    def GetObstacleForces(self):
        """Contact force on every coefficient (3 n_coef, the layout of f_ext) at the last gradient evaluation."""
        f = np.zeros(3 * self.n_coef)
        check(self._lib.tlfea_ancf_get_obstacle_forces(self._h, dp(f)))
        return f

    def GetObstacleResultant(self, k):
        """(force of obstacle k on the mesh as a 3-vector, sample points in contact) at the last gradient evaluation."""
        out = np.zeros(4)
        check(self._lib.tlfea_ancf_get_obstacle_resultant(self._h, int(k), dp(out)))
        return out[:3].copy(), int(round(out[3]))

    def GetSurfacePointWeights(self):
        """[E][32]: quadrature weight x reference surface Jacobian of every sample point; the sum is the sampled area."""
        w = np.zeros((self.n_elem, self.POINTS))
        check(self._lib.tlfea_ancf_get_surface_points(self._h, dp(w)))
        return w

    def GetSurfaceWeights(self):
        raise TypeError("GetSurfaceWeights is nodal (T10); an ANCF object has GetSurfacePointWeights")

    def RetrieveContactPointsToCPU(self):
        """[E][32][5]: x, y, z, smallest gap and normal pressure of every sample point at the current coefficients."""
        p = np.zeros((self.n_elem, self.POINTS, 5))
        check(self._lib.tlfea_ancf_retrieve_contact_points(self._h, dp(p)))
        return p


class GPU_ANCF3243_Data(_GPU_ANCF_Data):
    TYPE, KIND, NN, S, Q = "TYPE_3243", 3243, 2, 8, 12

    def Setup(self, length, width, height, gauss_xi_m, gauss_xi, gauss_eta, gauss_zeta, weight_xi_m, weight_xi,
              weight_eta, weight_zeta, h_x12, h_y12, h_z12, h_element_connectivity):
        """Argument order of ANCF3243Data.cuh:511-521 (the mass rule shares eta/zeta with the force rule)."""
        self._setup(length, width, height,
                    (gauss_xi_m, gauss_eta, gauss_zeta, weight_xi_m, weight_eta, weight_zeta),
                    (gauss_xi, gauss_eta, gauss_zeta, weight_xi, weight_eta, weight_zeta),
                    h_x12, h_y12, h_z12, h_element_connectivity)


class GPU_ANCF3443_Data(_GPU_ANCF_Data):
    TYPE, KIND, NN, S, Q = "TYPE_3443", 3443, 4, 16, 48

    def __init__(self, num_nodes, num_elements=None):
        """(num_nodes, num_elements), or the strip constructor (num_beams): every new shell of the chain brings two
        new nodes (ANCF3443Data.cuh:445-457)."""
        if num_elements is None:
            num_elements, num_nodes = int(num_nodes), 4 + 2 * (int(num_nodes) - 1)
        super().__init__(num_nodes, num_elements)

    def Setup(self, length, width, height, gauss_xi_m, gauss_eta_m, gauss_zeta_m, gauss_xi, gauss_eta, gauss_zeta,
              weight_xi_m, weight_eta_m, weight_zeta_m, weight_xi, weight_eta, weight_zeta, h_x12, h_y12, h_z12,
              element_connectivity):
        """Argument order of ANCF3443Data.cuh:532-542."""
        self._setup(length, width, height,
                    (gauss_xi_m, gauss_eta_m, gauss_zeta_m, weight_xi_m, weight_eta_m, weight_zeta_m),
                    (gauss_xi, gauss_eta, gauss_zeta, weight_xi, weight_eta, weight_zeta),
                    h_x12, h_y12, h_z12, element_connectivity)
