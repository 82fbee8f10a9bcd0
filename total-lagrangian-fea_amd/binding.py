"""ctypes binding of libtlfea_hip.so -- argument/return types for every symbol in include/tlfea_c.h."""
import ctypes as C
import importlib.util
import os
import re
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TLFEA_LIB_PATH") or os.path.join(_HERE, "libtlfea_hip.so")  # override: A/B experiments
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tlfea_c.h")
_LIB = None

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)
c_llp = C.POINTER(C.c_longlong)
HALO_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_ip, c_llp, c_llp)


class HaloListsC(C.Structure):  # tlfea_halo_lists
    _fields_ = [("n_peers", C.c_int), ("peers", c_ip), ("send_off", c_ip), ("send_nodes", c_ip), ("send_layer", c_ip),
                ("recv_off", c_ip), ("recv_nodes", c_ip), ("rank", C.c_int), ("world", C.c_int)]


class TlfeaError(RuntimeError):
    pass


class NewtonParams(C.Structure):  # SyncedNewtonParams (SyncedNewton.cuh:29-33)
    _fields_ = [("inner_atol", C.c_double), ("inner_rtol", C.c_double), ("outer_tol", C.c_double),
                ("rho", C.c_double), ("max_outer", C.c_int), ("max_inner", C.c_int), ("time_step", C.c_double)]


class AdamWParamsC(C.Structure):  # tlfea_adamw_params == SyncedAdamWParams (SyncedAdamW.cuh:27-34)
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("lr_decay", C.c_double), ("inner_tol", C.c_double),
                ("outer_tol", C.c_double), ("rho", C.c_double), ("max_outer", C.c_int), ("max_inner", C.c_int),
                ("time_step", C.c_double), ("convergence_check_interval", C.c_int), ("inner_rtol", C.c_double)]


class NesterovParamsC(C.Structure):  # tlfea_nesterov_params == SyncedNesterovParams (SyncedNesterov.cuh:26-30)
    _fields_ = [("alpha", C.c_double), ("rho", C.c_double), ("inner_tol", C.c_double), ("outer_tol", C.c_double),
                ("max_outer", C.c_int), ("max_inner", C.c_int), ("time_step", C.c_double)]


class VbdParamsC(C.Structure):  # tlfea_vbd_params == SyncedVBDParams (SyncedVBD.cuh:13-21)
    _fields_ = [("inner_tol", C.c_double), ("inner_rtol", C.c_double), ("outer_tol", C.c_double), ("rho", C.c_double),
                ("max_outer", C.c_int), ("max_inner", C.c_int), ("time_step", C.c_double), ("omega", C.c_double),
                ("hess_eps", C.c_double), ("convergence_check_interval", C.c_int), ("color_group_size", C.c_int)]


class LinSolveOptsC(C.Structure):
    _fields_ = [("rel_tol", C.c_double), ("max_iter", C.c_int), ("check_every", C.c_int), ("cheb_degree", C.c_int),
                ("cheb_kappa", C.c_double), ("cheb_bits", C.c_int), ("precond", C.c_int), ("method", C.c_int),
                ("on_unconverged", C.c_int)]


class ContactPatchC(C.Structure):  # tlfea_contact_patch == ContactPatch (HydroelasticNarrowphase.cuh)
    _fields_ = [("vertices", (C.c_double * 3) * 8), ("count", C.c_int), ("normal", C.c_double * 3),
                ("centroid", C.c_double * 3), ("area", C.c_double), ("g_A", C.c_double), ("g_B", C.c_double),
                ("p_equilibrium", C.c_double), ("tetA", C.c_int), ("tetB", C.c_int), ("isValid", C.c_int),
                ("validOrientation", C.c_int)]


class MaterialEntryC(C.Structure):  # tlfea_material_entry
    _fields_ = [(n, C.c_double) for n in ("E", "nu", "mu10", "mu01", "kappa", "rho0", "eta", "lamd")]


class ObstacleC(C.Structure):  # tlfea_obstacle
    _fields_ = [("kind", C.c_int), ("p", C.c_double * 3), ("n", C.c_double * 3), ("radius", C.c_double),
                ("vel", C.c_double * 3), ("stiffness", C.c_double), ("friction", C.c_double), ("eps_v", C.c_double)]


class FieldObstacleC(C.Structure):  # tlfea_field_obstacle
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("origin", C.c_double * 3), ("spacing", C.c_double),
                ("pos", C.c_double * 3), ("rot", C.c_double * 9), ("vel", C.c_double * 3), ("stiffness", C.c_double),
                ("friction", C.c_double), ("eps_v", C.c_double)]


class SurfaceLoadC(C.Structure):  # tlfea_surface_load
    _fields_ = [("kind", C.c_int), ("face", C.c_int), ("value", C.c_double * 3), ("scale", C.c_double),
                ("elems", c_ip), ("n_elems", C.c_int)]


class T10SurfaceLoadC(C.Structure):  # tlfea_t10_surface_load
    _fields_ = [("kind", C.c_int), ("value", C.c_double * 3), ("scale", C.c_double), ("faces", c_ip),
                ("n_faces", C.c_int)]


def _load_signatures(lib):
    """ctypes signatures of the distributed-load entry points."""
    vp, i = C.c_void_p, C.c_int
    sig = {"tlfea_set_body_acceleration": [vp, c_dp], "tlfea_ancf_set_surface_loads": [vp, C.POINTER(SurfaceLoadC), i],
           "tlfea_ancf_update_load_scale": [vp, i, C.c_double], "tlfea_clear_loads": [vp],
           "tlfea_get_load_forces": [vp, c_dp], "tlfea_get_load_resultant": [vp, c_dp],
           "tlfea_t10_get_boundary_faces": [vp, c_ip, c_ip, c_ip, c_ip],
           "tlfea_t10_set_surface_loads": [vp, C.POINTER(T10SurfaceLoadC), i],
           "tlfea_t10_update_load_scale": [vp, i, C.c_double]}
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int


def _obstacle_signatures(lib):
    """ctypes signatures of the rigid-obstacle entry points."""
    vp, i = C.c_void_p, C.c_int
    sig = {"tlfea_t10_set_obstacles": [vp, C.POINTER(ObstacleC), i],
           "tlfea_t10_update_obstacle": [vp, i, C.POINTER(ObstacleC)], "tlfea_t10_clear_obstacles": [vp],
           "tlfea_t10_get_obstacle_forces": [vp, c_dp], "tlfea_t10_get_obstacle_resultant": [vp, i, c_dp],
           "tlfea_t10_get_surface_weights": [vp, c_dp]}
    for name in list(sig)[:5]:  # the ANCF entry points (DESIGN 3e') take the same arguments
        sig[name.replace("tlfea_t10_", "tlfea_ancf_")] = sig[name]
    sig["tlfea_ancf_get_surface_points"] = [vp, c_dp]
    sig["tlfea_ancf_retrieve_contact_points"] = [vp, c_dp]
    # field obstacles (DESIGN 3e''), any handle
    sig["tlfea_set_field_obstacles"] = [vp, C.POINTER(FieldObstacleC), C.POINTER(c_dp), i]
    sig["tlfea_update_field_obstacle"] = [vp, i, C.POINTER(FieldObstacleC)]
    sig["tlfea_clear_field_obstacles"] = [vp]
    sig["tlfea_get_field_obstacle_resultant"] = [vp, i, c_dp]
    sig["tlfea_sdf_from_triangles"] = [c_dp, i, c_ip, i, i, i, i, c_dp, C.c_double, c_dp]
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int


def _stress_signatures(lib):
    """ctypes signatures of the stress-recovery entry points."""
    vp, i = C.c_void_p, C.c_int
    sig = {"tlfea_t10_calc_stress": [vp, vp, i], "tlfea_t10_calc_stress_host": [vp, c_dp, i],
           "tlfea_t10_retrieve_point_stress": [vp, c_dp],
           "tlfea_t10_retrieve_element_stress": [vp, c_dp, c_dp, c_dp, c_dp, c_dp],
           "tlfea_t10_retrieve_nodal_stress": [vp, c_dp, c_dp], "tlfea_t10_get_energies": [vp, c_dp],
           "tlfea_t10_time_stress_kernels": [vp, vp, i, i, c_dp]}
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int
    for name, args in sig.items():  # the ANCF entry points (DESIGN 3f') take the same arguments
        getattr(lib, name.replace("tlfea_t10_", "tlfea_ancf_")).argtypes = args
        getattr(lib, name.replace("tlfea_t10_", "tlfea_ancf_")).restype = C.c_int
    for name in ("tlfea_t10_nodal_stress_device_ptr", "tlfea_ancf_nodal_stress_device_ptr"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = vp


def _recovery_signatures(lib):
    """ctypes signatures of the recovered-stress entry points (DESIGN 3f'')."""
    vp, i = C.c_void_p, C.c_int
    sig = {"tlfea_t10_recover_stress": [vp, i, i], "tlfea_t10_recover_stress_from_points": [vp, c_dp, i, i],
           "tlfea_t10_retrieve_recovered_stress": [vp, c_dp, c_dp],
           "tlfea_t10_retrieve_principal_stress": [vp, c_dp, c_dp, c_dp, c_dp],
           "tlfea_t10_retrieve_error_indicator": [vp, c_dp, c_dp], "tlfea_t10_get_error_estimate": [vp, c_dp],
           "tlfea_t10_time_recovery_kernels": [vp, i, c_dp]}
    if not hasattr(lib, "tlfea_t10_recover_stress"):
        return  # an older build loaded through TLFEA_LIB_PATH (A/B runs) lacks these entry points
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int
    lib.tlfea_t10_recovered_stress_device_ptr.argtypes = [vp]
    lib.tlfea_t10_recovered_stress_device_ptr.restype = vp


def _material_signatures(lib):
    """ctypes signatures of the per-element material entry points."""
    vp, i = C.c_void_p, C.c_int
    sig = {"tlfea_t10_set_element_materials": [vp, i, i, C.POINTER(MaterialEntryC), c_ip, i],
           "tlfea_t10_clear_element_materials": [vp], "tlfea_t10_get_element_materials": [vp, c_ip, c_ip]}
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int


class ModalOptsC(C.Structure):  # tlfea_modal_opts
    _fields_ = [("n_modes", C.c_int), ("block_extra", C.c_int), ("shift", C.c_double), ("tol", C.c_double),
                ("max_iter", C.c_int), ("seed", C.c_uint)]


def _modal_signatures(lib):
    """ctypes signatures of the modal-analysis entry points."""
    vp, i = C.c_void_p, C.c_int
    sig = {"tlfea_newton_modal_solve": [vp, C.POINTER(ModalOptsC), c_dp, c_dp, c_dp, c_ip],
           "tlfea_newton_modal_apply_block": [vp, i, i, c_dp, c_dp, i],
           "tlfea_newton_modal_gram": [vp, i, i, c_dp, c_dp, c_dp],
           "tlfea_newton_modal_time_spmm": [vp, i, i, c_dp]}
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int


class AdjointInC(C.Structure):  # tlfea_adjoint_in (host or device pointers, by entry point)
    _fields_ = [(n, C.c_void_p) for n in ("x_bar", "v_bar", "lam_bar", "v_prev")]


class AdjointOutC(C.Structure):  # tlfea_adjoint_out
    _fields_ = [(n, C.c_void_p) for n in ("f_ext_bar", "v_prev_bar", "x_prev_bar", "lam_in_bar", "t_bar", "a_bar",
                                          "per_material", "per_element")]


def _adjoint_signatures(lib):
    """ctypes signatures of the adjoint-sensitivity entry points."""
    vp, i = C.c_void_p, C.c_int
    step = [vp, C.POINTER(AdjointInC), C.POINTER(AdjointOutC), c_ip, c_dp]
    sig = {"tlfea_newton_adjoint_step": step, "tlfea_newton_adjoint_step_device": step,
           "tlfea_newton_adjoint_ready": [vp], "tlfea_t10_material_sensitivity": [vp, c_dp, c_dp, c_dp, c_dp],
           "tlfea_t10_material_sensitivity_shape": [vp, c_ip, c_ip],
           "tlfea_t10_time_sensitivity_kernels": [vp, i, c_dp],
           # shape sensitivities: X_bar travels as an address (host or device, by entry point)
           "tlfea_newton_adjoint_step_shape": step[:3] + [vp] + step[3:],
           "tlfea_newton_adjoint_step_shape_device": step[:3] + [vp] + step[3:],
           "tlfea_t10_shape_sensitivity": [vp, c_dp, c_dp, c_dp], "tlfea_t10_time_shape_kernels": [vp, i, c_dp],
           "tlfea_t10_set_reference_positions": [vp, c_dp, c_dp, c_dp, i],
           # the ANCF kinds (DESIGN 3j')
           "tlfea_newton_ancf_adjoint_step": step, "tlfea_newton_ancf_adjoint_step_device": step,
           "tlfea_newton_ancf_adjoint_ready": [vp], "tlfea_ancf_material_sensitivity": [vp, c_dp, c_dp, c_dp, c_dp],
           "tlfea_ancf_material_sensitivity_shape": [vp, c_ip, c_ip], "tlfea_ancf_time_sensitivity_kernels": [vp, i, c_dp]}
    newer = {n for n in sig if "_shape" in n and n != "tlfea_t10_material_sensitivity_shape"} | {"tlfea_t10_set_reference_positions"}
    newer |= {n for n in sig if "ancf" in n}
    for name, args in sig.items():
        if name in newer and not hasattr(lib, name):
            continue  # an older build loaded through TLFEA_LIB_PATH (A/B runs) lacks the shape entry points
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int


def _pmg_signatures(lib):
    """ctypes signatures of the p-multigrid test hooks (the handle must not travel as a C int)."""
    vp = C.c_void_p
    sig = {"tlfea_newton_pmg_sizes": [vp, c_ip, c_ip],
           "tlfea_newton_pmg_retrieve": [vp, c_ip, c_ip, c_ip, c_ip, c_dp],
           "tlfea_newton_pmg_restrict_op_sizes": [vp, c_ip],
           "tlfea_newton_get_c32_geometry": [vp, C.c_int, c_ip],
           "tlfea_newton_get_direct_info": [vp, C.POINTER(C.c_longlong)],
           "tlfea_newton_get_direct_fronts": [vp, c_ip, c_ip],
           "tlfea_newton_cg_trace": [vp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_ip],
           "tlfea_newton_pmg_restrict_op_retrieve": [vp, c_ip, c_ip, c_dp],
           "tlfea_newton_pmg_fine_copy_retrieve": [vp, c_ip, c_ip, c_dp, c_dp, c_dp]}
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int
    if hasattr(lib, "tlfea_newton_get_assembly_form"):  # (as below: an older build lacks it)
        lib.tlfea_newton_get_assembly_form.argtypes = [vp, c_ip]
        lib.tlfea_newton_get_assembly_form.restype = C.c_int
    if hasattr(lib, "tlfea_newton_get_lambda_max"):  # an older build loaded through TLFEA_LIB_PATH (A/B runs) lacks it
        lib.tlfea_newton_get_lambda_max.argtypes = [vp, c_dp]
        lib.tlfea_newton_get_lambda_max.restype = C.c_int
    if hasattr(lib, "tlfea_newton_get_fine_smoother"):
        lib.tlfea_newton_get_fine_smoother.argtypes = [vp]
        lib.tlfea_newton_get_fine_smoother.restype = C.c_int
        c_fp = C.POINTER(C.c_float)
        lib.tlfea_newton_fine_smoother_pass.argtypes = [vp, c_fp, c_fp, c_fp, c_dp, c_dp, C.c_double, C.c_int, c_fp, c_fp, c_fp,
                                                        c_dp, c_dp]
        lib.tlfea_newton_fine_smoother_pass.restype = C.c_int
    if hasattr(lib, "tlfea_newton_get_setup_form"):
        lib.tlfea_newton_get_setup_form.argtypes = [vp, C.POINTER(C.c_longlong)]
        lib.tlfea_newton_get_setup_form.restype = C.c_int
        lib.tlfea_newton_get_setup_image.argtypes = [vp, c_dp, C.POINTER(C.c_longlong)]
        lib.tlfea_newton_get_setup_image.restype = C.c_int
        lib.tlfea_newton_get_block_diagonal.argtypes = [vp, c_dp]
        lib.tlfea_newton_get_block_diagonal.restype = C.c_int
    if hasattr(lib, "tlfea_newton_pmg_retrieve_built"):
        lib.tlfea_newton_pmg_retrieve_built.argtypes = [vp, c_dp, c_ip]
        lib.tlfea_newton_pmg_retrieve_built.restype = C.c_int
    if hasattr(lib, "tlfea_newton_get_fine_copy_state"):
        lib.tlfea_newton_get_fine_copy_state.argtypes = [vp, c_ip]
        lib.tlfea_newton_get_fine_copy_state.restype = C.c_int


def _contact_signatures(lib):
    """ctypes signatures of the tlfea_contact_* entry points (pointer arguments are c_void_p: device pointers pass as
    integers, host arrays through dp / ip)."""
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    sig = {"tlfea_contact_create": [i, i, i, c_ip, c_dp, c_ip, i, C.POINTER(C.c_void_p)],
           "tlfea_contact_destroy": [vp], "tlfea_contact_bind_t10": [vp, vp], "tlfea_contact_bind_nodes": [vp, vp, i],
           "tlfea_contact_step": [vp, vp, d, d], "tlfea_contact_set_base_force": [vp, c_dp, i],
           "tlfea_contact_apply_to_t10": [vp], "tlfea_contact_num_pairs": [vp, c_ip],
           "tlfea_contact_num_patches": [vp, c_ip], "tlfea_contact_retrieve_pairs": [vp, c_ip],
           "tlfea_contact_retrieve_patches": [vp, C.POINTER(ContactPatchC)], "tlfea_contact_retrieve_force": [vp, c_dp]}
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = C.c_int
    lib.tlfea_contact_force_device_ptr.argtypes = [vp]
    lib.tlfea_contact_force_device_ptr.restype = vp


def exported_symbols():
    """Names of every function declared in include/tlfea_c.h (parsed from the header)."""
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tlfea_[a-z0-9_]+)\s*\(", txt)) - {"tlfea_allreduce_fn"})


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 and link them by UNVERSIONED file name.  If
    this library has already mapped /opt/rocm's copies (soname libamdhip64.so.7), a later `import torch` therefore maps
    the wheel's copies as a SECOND HIP runtime in the process -- and that one finds no GPU ("No HIP GPUs are
    available").  Mapping the wheel's copies first makes both sides resolve to one runtime, in either import order.
    Nothing of torch is imported or executed here; TLFEA_SYSTEM_HIP=1 keeps /opt/rocm's runtime."""
    if "torch" in sys.modules or os.environ.get("TLFEA_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        pass  # no usable bundled runtime: the system one is used


def load_library():
    """dlopen the HIP library; fails loudly when it has not been built (no CPU path exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise TlfeaError(f"{LIB_PATH} is missing: build it with `make -C {_HERE}` "
                         "(or python -c 'import __graft_entry__ as g; g.build()').")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    lib.tlfea_last_error.restype = C.c_char_p
    for name in ("tlfea_t10_x12_device_ptr", "tlfea_t10_y12_device_ptr", "tlfea_t10_z12_device_ptr",
                 "tlfea_t10_external_force_device_ptr", "tlfea_t10_constraint_device_ptr",
                 "tlfea_newton_velocity_guess_device_ptr", "tlfea_adamw_velocity_guess_device_ptr", "tlfea_nesterov_velocity_guess_device_ptr",
                 "tlfea_vbd_velocity_guess_device_ptr"):
        getattr(lib, name).restype = C.c_void_p
        getattr(lib, name).argtypes = [C.c_void_p]
    _contact_signatures(lib)
    _material_signatures(lib)
    _obstacle_signatures(lib)
    _stress_signatures(lib)
    _recovery_signatures(lib)
    _load_signatures(lib)
    _modal_signatures(lib)
    _adjoint_signatures(lib)
    _pmg_signatures(lib)
    _LIB = lib
    return lib


def device_count():
    return load_library().tlfea_device_count()


def check(rc):
    if rc != 0:
        raise TlfeaError(load_library().tlfea_last_error().decode())


def dp(a):
    return a.ctypes.data_as(c_dp) if a is not None else None


def ip(a):
    return a.ctypes.data_as(c_ip) if a is not None else None
