"""ctypes binding of the C-ABI library (include/vamp_mvt_amd.h).

The library is the product: if it is missing or does not export every symbol the header declares, importing
this package fails loudly.  There is no Python/CPU fallback for any compute entry point.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# VMV_LIBRARY: developer override (ablation builds of the same ABI made by tools/); the product is the in-tree library
LIB_PATH = os.environ.get("VMV_LIBRARY") or os.path.join(_HERE, "libvamp_mvt_amd.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "vamp_mvt_amd.h")

c_float_p = ctypes.POINTER(ctypes.c_float)
c_u64_p = ctypes.POINTER(ctypes.c_uint64)
c_u32_p = ctypes.POINTER(ctypes.c_uint32)
c_size_p = ctypes.POINTER(ctypes.c_size_t)
c_u8_p = ctypes.POINTER(ctypes.c_uint8)

VMV_OK = 0
STATUS_NAMES = {0: "VMV_OK", 1: "VMV_ERR_INVALID_ARGUMENT", 2: "VMV_ERR_NO_DEVICE", 3: "VMV_ERR_HIP",
                4: "VMV_ERR_CAPACITY", 5: "VMV_ERR_NOT_FINALIZED", 6: "VMV_ERR_UNKNOWN_ROBOT", 7: "VMV_ERR_FINALIZED"}


class RrtcSettings(ctypes.Structure):
    """vmv_rrtc_settings"""
    _fields_ = [("range", ctypes.c_float), ("balance", ctypes.c_int), ("tree_ratio", ctypes.c_float),
                ("max_iterations", ctypes.c_uint32), ("max_samples", ctypes.c_uint32), ("check_every", ctypes.c_uint32)]


class RrtcGoalsSettings(ctypes.Structure):
    """vmv_rrtc_goals_settings"""
    _fields_ = [("base", RrtcSettings), ("dynamic_domain", ctypes.c_int), ("radius", ctypes.c_float), ("alpha", ctypes.c_float),
                ("min_radius", ctypes.c_float), ("start_tree_first", ctypes.c_int)]


class PrmSettings(ctypes.Structure):
    """vmv_prm_settings"""
    _fields_ = [("n_samples", ctypes.c_uint32), ("k", ctypes.c_uint32), ("radius", ctypes.c_float),
                ("keep_roadmaps", ctypes.c_int)]


class RoadmapSettings(ctypes.Structure):
    """vmv_roadmap_settings"""
    _fields_ = [("n_samples", ctypes.c_uint32), ("k", ctypes.c_uint32), ("radius", ctypes.c_float)]


class RoadmapQuerySettings(ctypes.Structure):
    """vmv_roadmap_query_settings"""
    _fields_ = [("k_connect", ctypes.c_uint32), ("radius", ctypes.c_float)]


class FcitSettings(ctypes.Structure):
    """vmv_fcit_settings"""
    _fields_ = [("n_samples", ctypes.c_uint32), ("max_iterations", ctypes.c_uint32), ("questions_per_round", ctypes.c_uint32),
                ("check_every", ctypes.c_uint32)]


class SimplifySettings(ctypes.Structure):
    """vmv_simplify_settings"""
    _fields_ = [("max_iterations", ctypes.c_uint32), ("interpolate", ctypes.c_uint32), ("n_operations", ctypes.c_uint32),
                ("operations", ctypes.c_uint32 * 8), ("bspline_max_steps", ctypes.c_uint32),
                ("bspline_min_change", ctypes.c_float), ("bspline_midpoint_interpolation", ctypes.c_float),
                ("max_waypoints", ctypes.c_uint32), ("questions_per_round", ctypes.c_uint32), ("check_every", ctypes.c_uint32)]


class OptimizeSettings(ctypes.Structure):
    """vmv_optimize_settings"""
    _fields_ = [("max_iterations", ctypes.c_uint32), ("validate_every", ctypes.c_uint32), ("step", ctypes.c_float),
                ("max_step", ctypes.c_float), ("min_change", ctypes.c_float), ("smooth_weight", ctypes.c_float),
                ("env_weight", ctypes.c_float), ("self_weight", ctypes.c_float), ("env_margin", ctypes.c_float),
                ("self_margin", ctypes.c_float), ("max_waypoints", ctypes.c_uint32)]


class AorrtcSettings(ctypes.Structure):
    """vmv_aorrtc_settings"""
    _fields_ = [("rrtc", RrtcSettings), ("simplify", SimplifySettings), ("optimize", ctypes.c_int),
                ("cost_bound_resample", ctypes.c_int), ("simplify_intermediate", ctypes.c_int),
                ("max_iterations", ctypes.c_uint32), ("max_internal_iterations", ctypes.c_uint32),
                ("max_samples", ctypes.c_uint32), ("max_cost_bound_resamples", ctypes.c_uint32), ("max_searches", ctypes.c_uint32)]


class IkSettings(ctypes.Structure):
    """vmv_ik_settings"""
    _fields_ = [("n_seeds", ctypes.c_uint32), ("max_iterations", ctypes.c_uint32), ("pos_tol", ctypes.c_float),
                ("rot_tol", ctypes.c_float), ("rot_weight", ctypes.c_float), ("damping", ctypes.c_float),
                ("max_step", ctypes.c_float), ("position_only", ctypes.c_int)]


class EeConstraint(ctypes.Structure):
    """vmv_ee_constraint"""
    _fields_ = [("frame", ctypes.c_float * 16), ("pos_lo", ctypes.c_float * 3), ("pos_hi", ctypes.c_float * 3),
                ("tool_axis", ctypes.c_float * 3), ("ref_axis", ctypes.c_float * 3), ("max_angle", ctypes.c_float)]


class ConstraintSettings(ctypes.Structure):
    """vmv_constraint_settings"""
    _fields_ = [("max_iterations", ctypes.c_uint32), ("pos_tol", ctypes.c_float), ("rot_tol", ctypes.c_float),
                ("rot_weight", ctypes.c_float), ("damping", ctypes.c_float), ("max_step", ctypes.c_float),
                ("check_step", ctypes.c_float)]


class ConstraintPlanSettings(ctypes.Structure):
    """vmv_constraint_plan_settings"""
    _fields_ = [("base", ConstraintSettings), ("max_stretch", ctypes.c_float)]


class CartesianSettings(ctypes.Structure):
    """vmv_cartesian_settings"""
    _fields_ = [("pos_step", ctypes.c_float), ("rot_step", ctypes.c_float), ("max_iterations", ctypes.c_uint32),
                ("pos_tol", ctypes.c_float), ("rot_tol", ctypes.c_float), ("rot_weight", ctypes.c_float),
                ("damping", ctypes.c_float), ("max_step", ctypes.c_float), ("max_joint_step", ctypes.c_float),
                ("max_waypoints", ctypes.c_uint32), ("position_only", ctypes.c_int)]


class RetimeSettings(ctypes.Structure):
    """vmv_retime_settings"""
    _fields_ = [("blend", ctypes.c_float), ("grid_step", ctypes.c_float), ("dt", ctypes.c_float),
                ("max_grid", ctypes.c_uint32), ("max_samples", ctypes.c_uint32), ("stop_at_waypoints", ctypes.c_int)]


class RetimeConstrainedSettings(ctypes.Structure):
    """vmv_retime_constrained_settings"""
    _fields_ = [("base", RetimeSettings), ("blend_halvings", ctypes.c_uint32), ("max_rounds", ctypes.c_uint32)]


class VmvError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__(f"{where}: {STATUS_NAMES.get(status, status)}" + (f" ({detail})" if detail else ""))


def declared_symbols(header_path: str = HEADER_PATH):
    """Every function name include/vamp_mvt_amd.h declares."""
    with open(header_path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vmv_[a-z0-9_]+)\s*\(", text)))


def _load():
    # PyTorch-ROCm bundles its own HIP runtime.  Two HIP runtimes in one process fight over the device
    # ("No HIP GPUs are available" in whichever initialises second), so when torch is installed its runtime is
    # loaded first and this library binds to the same libamdhip64 (torch stays plumbing: memory, streams, RCCL).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
            "vamp_mvt_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"{LIB_PATH} does not export: {', '.join(missing)}")
    V, I, F, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    sig = {
        "vmv_status_string": (ctypes.c_char_p, [I]),
        "vmv_abi_version": (I, []),
        "vmv_last_error": (ctypes.c_char_p, []),
        "vmv_device_count": (I, [ctypes.POINTER(I)]),
        "vmv_set_device": (I, [I]),
        "vmv_get_device": (I, [ctypes.POINTER(I)]),
        "vmv_num_robots": (I, []),
        "vmv_robot_name": (ctypes.c_char_p, [I]),
        "vmv_robot_id": (I, [ctypes.c_char_p]),
        "vmv_robot_dimension": (I, [I]),
        "vmv_robot_n_spheres": (I, [I]),
        "vmv_robot_resolution": (I, [I]),
        "vmv_robot_min_max_radii": (I, [I, c_float_p, c_float_p]),
        "vmv_robot_bounds": (I, [I, c_float_p, c_float_p, c_float_p]),
        "vmv_robot_joint_name": (ctypes.c_char_p, [I, I]),
        "vmv_robot_end_effector": (ctypes.c_char_p, [I]),
        "vmv_env_create": (I, [ctypes.POINTER(V)]),
        "vmv_env_destroy": (I, [V]),
        "vmv_env_add_sphere": (I, [V, F, F, F, F]),
        "vmv_env_add_cuboid": (I, [V, c_float_p]),
        "vmv_env_add_capsule": (I, [V, c_float_p]),
        "vmv_filter_pointcloud": (I, [c_float_p, S, F, F, F, c_float_p, c_float_p, c_float_p, I, I, c_float_p, S, c_size_p,
                                      c_u64_p, c_u64_p]),
        "vmv_env_add_capt_pointcloud_gpu": (I, [V, c_float_p, S, F, F, F, c_u64_p, c_u64_p]),
        "vmv_env_add_heightfield": (I, [V, c_float_p, c_float_p, S, S, c_float_p]),
        "vmv_env_heightfield_count": (I, [V, c_size_p]),
        "vmv_env_add_capt_pointcloud": (I, [V, c_float_p, S, F, F, F, c_u64_p]),
        "vmv_env_add_mvt_pointcloud": (I, [V, c_float_p, S, F, F, c_float_p, c_float_p, F, c_u64_p, ctypes.POINTER(I)]),
        "vmv_env_mvt_count": (I, [V, c_size_p]),
        "vmv_env_mvt_info": (I, [V, S, c_u32_p, c_u32_p, c_u32_p, c_float_p, c_float_p]),
        "vmv_env_finalize": (I, [V]),
        "vmv_env_counts": (I, [V, c_size_p]),
        "vmv_env_get_spheres": (I, [V, c_float_p, S, c_size_p]),
        "vmv_env_get_cuboids": (I, [V, I, c_float_p, S, c_size_p]),
        "vmv_env_get_capsules": (I, [V, I, c_float_p, S, c_size_p]),
        "vmv_env_capt_sizes": (I, [V, S, c_u32_p, c_u32_p]),
        "vmv_env_capt_arrays": (I, [V, S, c_float_p, c_u32_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p]),
        "vmv_fk_batch": (I, [I, V, S, V, V]),
        "vmv_validate_batch": (I, [I, V, V, S, V, V]),
        "vmv_validate_batch_env": (I, [I, V, V, S, V, V]),
        "vmv_validate_batch_self": (I, [I, V, S, V, V]),
        "vmv_self_screen_flags": (I, [I, V, S, I, V, V]),
        "vmv_bare_trig_error": (I, [ctypes.c_uint32, ctypes.c_uint32, c_float_p, V]),
        "vmv_validate_motion_batch": (I, [I, V, V, V, S, V, V]),
        "vmv_fk_batch_host": (I, [I, c_float_p, S, c_float_p]),
        "vmv_eefk_batch": (I, [I, V, S, V, V]),
        "vmv_contacts_batch_host": (I, [I, V, c_float_p, S, c_u32_p, c_u32_p]),
        "vmv_env_report_layout": (I, [V, c_u32_p]),
        "vmv_robot_self_pairs": (I, [I, c_size_p, ctypes.POINTER(ctypes.c_uint16)]),
        "vmv_eefk_batch_host": (I, [I, c_float_p, S, c_float_p]),
        "vmv_env_attach": (I, [V, c_float_p, c_float_p, S]),
        "vmv_env_detach": (I, [V]),
        "vmv_filter_self_from_pointcloud": (I, [I, V, c_float_p, c_float_p, S, F, c_float_p, S, c_size_p]),
        "vmv_shard_range": (I, [S, I, I, c_size_p, c_size_p]),
        "vmv_shard_words": (S, [S, I]),
        "vmv_spheres_in_collision_batch": (I, [V, V, S, V, V]),
        "vmv_spheres_in_collision_batch_host": (I, [V, c_float_p, S, c_u8_p]),
        "vmv_validate_batch_host": (I, [I, V, c_float_p, S, c_u64_p]),
        "vmv_validate_batch_multi": (I, [I, ctypes.POINTER(V), c_size_p, S, V, V, V]),
        "vmv_validate_batch_multi_host": (I, [I, ctypes.POINTER(V), c_size_p, S, c_float_p, c_u64_p]),
        "vmv_validate_motion_batch_host": (I, [I, V, c_float_p, c_float_p, S, c_u64_p]),
        "vmv_validate_motion_batch_multi": (I, [I, ctypes.POINTER(V), c_size_p, S, V, V, V, V]),
        "vmv_validate_motion_batch_multi_host": (I, [I, ctypes.POINTER(V), c_size_p, S, c_float_p, c_float_p, c_u64_p]),
        "vmv_clearance_batch": (I, [I, V, V, S, V, V, V]),
        "vmv_clearance_batch_host": (I, [I, V, c_float_p, S, c_float_p, c_u32_p]),
        "vmv_clearance_batch_multi": (I, [I, ctypes.POINTER(V), c_size_p, S, V, V, V, V]),
        "vmv_clearance_batch_multi_host": (I, [I, ctypes.POINTER(V), c_size_p, S, c_float_p, c_float_p, c_u32_p]),
        "vmv_clearance_grad_batch": (I, [I, V, V, S, V, V, V, V]),
        "vmv_clearance_grad_batch_host": (I, [I, V, c_float_p, S, c_float_p, c_float_p, c_u32_p]),
        "vmv_clearance_grad_batch_multi": (I, [I, ctypes.POINTER(V), c_size_p, S, V, V, V, V, V]),
        "vmv_clearance_grad_batch_multi_host": (I, [I, ctypes.POINTER(V), c_size_p, S, c_float_p, c_float_p, c_float_p,
                                                    c_u32_p]),
        "vmv_eefk_jacobian_batch": (I, [I, V, S, V, V, V]),
        "vmv_eefk_jacobian_batch_host": (I, [I, c_float_p, S, c_float_p, c_float_p]),
        "vmv_ik_batch": (I, [I, V, S, V, ctypes.c_uint64, ctypes.POINTER(IkSettings), V, V, V, V]),
        "vmv_ik_batch_host": (I, [I, c_float_p, S, c_float_p, ctypes.c_uint64, ctypes.POINTER(IkSettings), c_float_p, c_float_p,
                                  c_u32_p]),
        "vmv_constraint_project_batch": (I, [I, V, S, ctypes.POINTER(EeConstraint), S, ctypes.POINTER(ConstraintSettings), V, V, V, V]),
        "vmv_constraint_project_batch_host": (I, [I, c_float_p, S, ctypes.POINTER(EeConstraint), S, ctypes.POINTER(ConstraintSettings),
                                                  c_float_p, c_float_p, c_u32_p]),
        "vmv_constraint_check_batch": (I, [I, V, S, ctypes.POINTER(EeConstraint), S, ctypes.POINTER(ConstraintSettings), V, V, V]),
        "vmv_constraint_check_batch_host": (I, [I, c_float_p, S, ctypes.POINTER(EeConstraint), S, ctypes.POINTER(ConstraintSettings),
                                                c_u64_p, c_float_p]),
        "vmv_constraint_check_motion_batch": (I, [I, V, V, S, ctypes.POINTER(EeConstraint), S, ctypes.POINTER(ConstraintSettings), V, V]),
        "vmv_constraint_check_motion_batch_host": (I, [I, c_float_p, c_float_p, S, ctypes.POINTER(EeConstraint), S,
                                                       ctypes.POINTER(ConstraintSettings), c_u8_p]),
        "vmv_env_prepare_multi": (I, [I, ctypes.POINTER(V), S]),
        "vmv_rrtc_multi": (I, [I, ctypes.POINTER(V), S, c_float_p, c_float_p, c_u64_p, ctypes.POINTER(RrtcSettings),
                               ctypes.POINTER(V)]),
        "vmv_rrtc_multi_goals": (I, [I, ctypes.POINTER(V), S, c_float_p, c_float_p, c_size_p, c_u64_p,
                                     ctypes.POINTER(RrtcGoalsSettings), ctypes.POINTER(V)]),
        "vmv_rrtc_multi_constrained": (I, [I, ctypes.POINTER(V), S, c_float_p, c_float_p, c_size_p, c_u64_p,
                                           ctypes.POINTER(RrtcGoalsSettings), ctypes.POINTER(EeConstraint), S,
                                           ctypes.POINTER(ConstraintPlanSettings), ctypes.POINTER(V)]),
        "vmv_plans_goal_indices": (I, [V, c_u32_p]),
        "vmv_plans_band_refused": (I, [V, c_u32_p]),
        "vmv_plans_summary": (I, [V, c_u8_p, c_u32_p, c_u32_p, c_u32_p, c_u64_p, c_u64_p]),
        "vmv_plans_paths": (I, [V, c_float_p, S]),
        "vmv_plans_destroy": (I, [V]),
        "vmv_prm_multi": (I, [I, ctypes.POINTER(V), S, c_float_p, c_float_p, c_u64_p, c_float_p, ctypes.POINTER(PrmSettings),
                              ctypes.POINTER(V)]),
        "vmv_plans_roadmap_summary": (I, [V, c_u32_p, c_u32_p, c_u32_p, c_float_p]),
        "vmv_plans_roadmap_vertices": (I, [V, S, c_u8_p]),
        "vmv_plans_roadmap_edges": (I, [V, S, c_u32_p, c_u8_p, S, c_size_p]),
        "vmv_roadmaps_build": (I, [I, ctypes.POINTER(V), S, c_u64_p, c_float_p, ctypes.POINTER(RoadmapSettings), ctypes.POINTER(V)]),
        "vmv_roadmaps_query": (I, [V, S, c_u32_p, c_float_p, c_float_p, ctypes.POINTER(RoadmapQuerySettings), ctypes.POINTER(V)]),
        "vmv_plans_query_summary": (I, [V, c_float_p, c_u32_p]),
        "vmv_roadmaps_summary": (I, [V, c_u32_p, c_u32_p, c_u32_p]),
        "vmv_roadmaps_vertices": (I, [V, S, c_float_p, c_u8_p]),
        "vmv_roadmaps_edges": (I, [V, S, c_u32_p, c_u8_p, S, c_size_p]),
        "vmv_roadmaps_destroy": (I, [V]),
        "vmv_aorrtc_multi": (I, [I, ctypes.POINTER(V), S, c_float_p, c_float_p, c_u64_p, ctypes.POINTER(AorrtcSettings),
                                 ctypes.POINTER(V)]),
        "vmv_aorrtc_multi_constrained": (I, [I, ctypes.POINTER(V), S, c_float_p, c_float_p, c_u64_p, ctypes.POINTER(AorrtcSettings),
                                             ctypes.POINTER(EeConstraint), S, ctypes.POINTER(ConstraintPlanSettings),
                                             ctypes.POINTER(V)]),
        "vmv_plans_costs": (I, [V, c_float_p, c_float_p, c_u32_p, c_u32_p]),
        "vmv_fcit_multi": (I, [I, ctypes.POINTER(V), S, c_float_p, c_float_p, c_u64_p, c_float_p, ctypes.POINTER(FcitSettings),
                               ctypes.POINTER(V)]),
        "vmv_plans_fcit_summary": (I, [V, c_float_p, c_u32_p]),
        "vmv_phs_samples": (I, [I, c_float_p, c_float_p, F, ctypes.c_uint32, ctypes.c_uint32, S, c_float_p, c_u8_p, c_u32_p]),
        "vmv_simplify_multi": (I, [I, ctypes.POINTER(V), S, c_float_p, c_size_p, ctypes.POINTER(SimplifySettings),
                                   ctypes.POINTER(V)]),
        "vmv_simplify_multi_constrained": (I, [I, ctypes.POINTER(V), S, c_float_p, c_size_p, ctypes.POINTER(SimplifySettings),
                                               ctypes.POINTER(EeConstraint), S, ctypes.POINTER(ConstraintSettings),
                                               ctypes.POINTER(V)]),
        "vmv_paths_band_refused": (I, [V, c_u32_p]),
        "vmv_paths_summary": (I, [V, c_u8_p, c_u32_p, c_u32_p, c_u32_p, c_u64_p, c_u64_p]),
        "vmv_paths_points": (I, [V, c_float_p, S]),
        "vmv_paths_destroy": (I, [V]),
        "vmv_optimize_multi": (I, [I, ctypes.POINTER(V), S, c_float_p, c_size_p, ctypes.POINTER(OptimizeSettings),
                                   ctypes.POINTER(V)]),
        "vmv_optimized_summary": (I, [V, c_u8_p, c_u32_p, c_u32_p, c_float_p, c_float_p, c_float_p, c_float_p, c_u64_p, c_u64_p]),
        "vmv_optimized_points": (I, [V, c_float_p, S]),
        "vmv_optimized_destroy": (I, [V]),
        "vmv_optimize_multi_constrained": (I, [I, ctypes.POINTER(V), S, c_float_p, c_size_p, ctypes.POINTER(OptimizeSettings),
                                               ctypes.POINTER(EeConstraint), S, ctypes.POINTER(ConstraintSettings),
                                               ctypes.POINTER(V)]),
        "vmv_optimized_held": (I, [V, c_u32_p]),
        "vmv_cartesian_multi": (I, [I, ctypes.POINTER(V), S, c_float_p, c_float_p, ctypes.POINTER(CartesianSettings),
                                    ctypes.POINTER(V)]),
        "vmv_cartesian_summary": (I, [V, c_u8_p, c_u32_p, c_u32_p, c_u32_p, c_u64_p, c_u64_p]),
        "vmv_cartesian_points": (I, [V, c_float_p, S]),
        "vmv_cartesian_destroy": (I, [V]),
        "vmv_retime_multi": (I, [I, ctypes.POINTER(V), S, c_float_p, c_size_p, c_float_p, c_float_p,
                                 ctypes.POINTER(RetimeSettings), ctypes.POINTER(V)]),
        "vmv_retime_summary": (I, [V, c_u8_p, c_u32_p, c_u32_p, c_float_p, c_u32_p, c_u64_p, c_u64_p]),
        "vmv_retime_samples": (I, [V, c_float_p, c_float_p, c_float_p, c_float_p, S]),
        "vmv_retime_destroy": (I, [V]),
        "vmv_retime_multi_constrained": (I, [I, ctypes.POINTER(V), S, c_float_p, c_size_p, c_float_p, c_float_p,
                                             ctypes.POINTER(EeConstraint), S, ctypes.POINTER(RetimeConstrainedSettings),
                                             ctypes.POINTER(ConstraintSettings), ctypes.POINTER(V)]),
        "vmv_retime_levels": (I, [V, c_u8_p, c_u32_p, c_u32_p, c_u32_p]),
        # (exported for the tests only; not declared in the public header)
        "vmv_retime_band_pairs_host": (I, [I, c_float_p, c_size_p, S, ctypes.POINTER(EeConstraint), S,
                                           ctypes.POINTER(ConstraintSettings), c_u8_p]),
        "vmv_env_grid_info": (I, [V, I, I, c_u32_p, c_float_p, c_float_p, c_u32_p]),
        "vmv_env_grid_cells": (I, [V, I, I, c_u32_p, S, c_size_p]),
        "vmv_env_robot_flags": (I, [V, I, c_u64_p, c_u32_p]),
        "vmv_release_staging": (I, []),
        "vmv_halton_configs": (I, [I, ctypes.c_uint64, V, S, V]),
        "vmv_time_validate_batch": (I, [I, V, V, S, V, I, V, c_float_p]),
        "vmv_fill_uniform_configs": (I, [I, V, S, ctypes.c_uint64, V]),
        "vmv_kernel_name": (ctypes.c_char_p, [I, ctypes.c_char_p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(status: int, where: str):
    if status != VMV_OK:
        raise VmvError(status, where, lib.vmv_last_error().decode(errors="replace"))
