"""ctypes binding of libhyteg_host.so (include/hyteg_host.h): the C facade of the C++ host layer
(hyteg_amd/host/hyteg_host.hpp) that mirrors HyTeG's PrimitiveStorage / P1Function / P1ConstantLaplaceOperator /
grid transfer / solver classes.  Used by the tests, bench.py and the torch.distributed driver; plumbing only."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import NamedTuple

import numpy as np

_PKG = Path(__file__).resolve().parent
_LIB_PATH = _PKG / "lib" / "libhyteg_host.so"

Inner, DirichletBoundary, NeumannBoundary, FreeslipBoundary, All, Boundary = 1, 2, 4, 8, 15, 14
Replace, Add = 0, 1
JACOBI, GAUSS_SEIDEL, SOR, JACOBI_FP32 = 0, 1, 2, 3  # JACOBI_FP32: MixedPrecisionJacobiSmoother (float sweeps on cell interiors)
SYMMETRIC_GAUSS_SEIDEL, SYMMETRIC_SOR = 5, 6  # a forward sweep followed by a backward one (SymmetricSORSmoother.hpp)
IDENTITY = -1  # IdentityPreconditioner, for Solver.smoother / P2Solver.smoother only
CHEBYSHEV = 4  # ChebyshevSmoother: not a code of hyteg_host_gmg_create (it has its own entry points: Solver.chebyshev / gmg_chebyshev)

_vp, _i, _d, _u = C.c_void_p, C.c_int, C.c_double, C.c_uint
_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
EXCHANGE_CB = C.CFUNCTYPE(_i, _vp, _i, _i)
ALLREDUCE_CB = C.CFUNCTYPE(_i, _vp, _dp, _i)
LOCATION_CB = C.CFUNCTYPE(_i, _vp, _dp)  # the predicate of set_mesh_boundary_flags_by_*_location: (user, xyz) -> 0 / 1
_ull = C.c_ulonglong
NORMAL_CB = C.CFUNCTYPE(_i, _vp, _dp, _dp)  # hh_normal_callback_t: (user, xyz, normal out) -> 0, the normal function of the projection
LEVEL_CB = C.CFUNCTYPE(None, C.c_uint64, _vp)  # hh_level_callback_t: the callbacks of FullMultigridSolver

SIGNATURES = {
    "hyteg_host_last_error": (C.c_char_p, []),
    "hyteg_host_storage_from_gmsh": (_i, [C.c_char_p, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_storage_from_arrays": (_i, [_i, _dp, _i, _ip, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_storage_destroy": (_i, [_vp]),
    "hyteg_host_storage_counts": (_i, [_vp, _ip]),
    "hyteg_host_storage_local_cell": (_i, [_vp, _i, _ip, _dp, _dp]),
    "hyteg_host_storage_mask": (_i, [_vp, _i, _i, _i, C.POINTER(_u)]),
    "hyteg_host_storage_set_boundary_type": (_i, [_vp, _i]),
    "hyteg_host_storage_mask_bc": (_i, [_vp, _i, _i, _i, _vp, C.POINTER(_u)]),
    "hyteg_host_storage_set_mesh_boundary_flags_on_boundary": (_i, [_vp, _ull, _ull, _i]),
    "hyteg_host_storage_set_mesh_boundary_flags_inner": (_i, [_vp, _ull, _i]),
    "hyteg_host_storage_set_mesh_boundary_flags_by_vertex_location": (_i, [_vp, _ull, LOCATION_CB, _vp, _i]),
    "hyteg_host_storage_set_mesh_boundary_flags_by_centroid_location": (_i, [_vp, _ull, LOCATION_CB, _vp]),
    "hyteg_host_storage_set_mesh_boundary_flag": (_i, [_vp, _i, _i, _ull]),
    "hyteg_host_storage_primitive": (_i, [_vp, _i, _i, _ip, _ip, _dp, C.POINTER(_ull), _ip]),
    "hyteg_host_storage_boundary_classes": (_i, [_vp, _ip, C.POINTER(_ull)]),
    "hyteg_host_storage_default_boundary_condition": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_boundary_condition_create": (_i, [_i, C.POINTER(_vp)]),
    "hyteg_host_boundary_condition_destroy": (_i, [_vp]),
    "hyteg_host_boundary_condition_create_domain": (_i, [_vp, C.c_char_p, _i, _i, C.POINTER(_ull), _ip]),
    "hyteg_host_boundary_condition_type": (_i, [_vp, _ull, _ip]),
    "hyteg_host_boundary_condition_uid": (_i, [_vp, _ull, _ip, C.c_char_p, _i]),
    "hyteg_host_boundary_condition_equal": (_i, [_vp, _vp, _ip]),
    "hyteg_host_function_set_boundary_condition": (_i, [_vp, _vp]),
    "hyteg_host_function_boundary_condition": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_function_interpolate_constant_on_boundary": (_i, [_vp, _d, _i, _i, C.c_char_p]),
    "hyteg_host_p2function_set_boundary_condition": (_i, [_vp, _vp]),
    "hyteg_host_p2function_boundary_condition": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_p2function_interpolate_constant_on_boundary": (_i, [_vp, _d, _i, _i, C.c_char_p]),
    "hyteg_host_storage_set_stream": (_i, [_vp, _vp]),
    "hyteg_host_storage_set_batch_max_level": (_i, [_vp, _i]),
    "hyteg_host_storage_set_apply_lanes": (_i, [_vp, _i]),
    "hyteg_host_storage_set_apply_cell_lanes_min": (_i, [_vp, _i]),
    "hyteg_host_storage_lanes_seen": (_i, [_vp, C.POINTER(C.c_uint)]),
    "hyteg_host_storage_set_apply_steps": (_i, [_vp, _i]),
    "hyteg_host_storage_steps_launches": (_i, [_vp, C.POINTER(_u)]),
    "hyteg_host_apply_steps_plan": (_i, [_i, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), _i, _i, _i, _i, _ip, _ip]),
    "hyteg_host_lane_plan": (_i, [_i, _i, _ip, C.POINTER(C.c_ulonglong), _ip, C.POINTER(C.c_ulonglong), _ip, C.POINTER(_u)]),
    "hyteg_host_storage_set_hooks": (_i, [_vp, EXCHANGE_CB, EXCHANGE_CB, ALLREDUCE_CB, _vp]),
    "hyteg_host_storage_use_rccl": (_i, [_vp, C.c_char_p]),
    "hyteg_host_storage_use_p2p": (_i, [_vp, C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "hyteg_host_storage_p2p_open": (_i, [_vp, C.c_char_p]),
    "hyteg_host_storage_p2p_layout": (_i, [_vp, _i, _i, C.POINTER(C.c_longlong)]),
    "hyteg_host_storage_p2p_connect": (_i, [_vp, _i, _i, C.POINTER(C.c_longlong)]),
    "hyteg_host_storage_drop_p2p": (_i, [_vp]),
    "hyteg_host_storage_check_transport": (_i, [_vp]),
    "hyteg_host_storage_transport_name": (_i, [_vp, C.c_char_p, _i]),
    "hyteg_host_storage_allreduce_sum": (_i, [_vp, _dp, _i]),
    "hyteg_host_storage_allreduce_max": (_i, [_vp, _dp, _i]),
    "hyteg_host_storage_p1_number_of_dofs": (_i, [_vp, _i, _i, C.POINTER(C.c_ulonglong)]),
    "hyteg_host_storage_p2_number_of_dofs": (_i, [_vp, _i, _i, C.POINTER(C.c_ulonglong)]),
    "hyteg_host_p1_reduce": (_i, [_vp, _i, _i, _i, _dp]),
    "hyteg_host_p2_reduce": (_i, [_vp, _i, _i, _i, _dp]),
    "hyteg_host_storage_enable_timing": (_i, [_vp, _i, _i]),
    "hyteg_host_storage_timing_json": (_i, [_vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hyteg_host_storage_timing_reset": (_i, [_vp]),
    "hyteg_host_plan_sizes": (_i, [_vp, _i, _i, _ip]),
    "hyteg_host_plan_export": (_i, [_vp, _i, _i, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _ip]),
    "hyteg_host_plan_register_buffers": (_i, [_vp, _i, _i, _vp, _vp]),
    "hyteg_host_function_create": (_i, [_vp, C.c_char_p, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_function_destroy": (_i, [_vp]),
    "hyteg_host_function_cell_pointer": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_function_upload_cell": (_i, [_vp, _i, _i, _dp]),
    "hyteg_host_function_download_cell": (_i, [_vp, _i, _i, _dp]),
    "hyteg_host_function_interpolate_constant": (_i, [_vp, _d, _i, _i]),
    "hyteg_host_function_assign": (_i, [_vp, _i, _dp, C.POINTER(_vp), _i, _i]),
    "hyteg_host_function_add": (_i, [_vp, _i, _dp, C.POINTER(_vp), _i, _i]),
    "hyteg_host_function_mult_elementwise": (_i, [_vp, _i, C.POINTER(_vp), _i, _i]),
    "hyteg_host_function_dot": (_i, [_vp, _vp, _i, _i, _i, _dp]),
    "hyteg_host_function_sum_shared": (_i, [_vp, _i, _i]),
    "hyteg_host_function_sync_shared": (_i, [_vp, _i, _i]),
    "hyteg_host_function_set_all_inner": (_i, [_vp, _i]),
    "hyteg_host_th_function_create": (_i, [_vp, C.c_char_p, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_th_function_destroy": (_i, [_vp]),
    "hyteg_host_th_function_velocity": (_i, [_vp, _i, C.POINTER(_vp)]),
    "hyteg_host_th_function_pressure": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_th_function_assign": (_i, [_vp, _i, _dp, C.POINTER(_vp), _i, _i]),
    "hyteg_host_th_function_interpolate_constant": (_i, [_vp, _d, _i, _i]),
    "hyteg_host_th_function_dot": (_i, [_vp, _vp, _i, _i, C.POINTER(_d)]),
    "hyteg_host_th_operator_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_th_operator_destroy": (_i, [_vp]),
    "hyteg_host_th_operator_apply": (_i, [_vp, _vp, _vp, _i, _i]),
    "hyteg_host_th_operator_apply_block": (_i, [_vp, _i, _vp, _vp, _i, _i]),
    "hyteg_host_th_gmg_create": (_i, [_vp, _i, _i, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_th_minres_create": (_i, [_vp, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_th_solver_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_th_solver_destroy": (_i, [_vp]),
    "hyteg_host_th_project_pressure_mean": (_i, [_vp, _i]),
    "hyteg_host_th_form_element_matrix": (_i, [_i, _i, _dp, _dp]),
    "hyteg_host_stokes_function_create": (_i, [_vp, C.c_char_p, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_stokes_function_destroy": (_i, [_vp]),
    "hyteg_host_stokes_function_component": (_i, [_vp, _i, C.POINTER(_vp)]),
    "hyteg_host_stokes_function_assign": (_i, [_vp, _i, _dp, C.POINTER(_vp), _i, _i]),
    "hyteg_host_stokes_function_dot": (_i, [_vp, _vp, _i, _i, _dp]),
    "hyteg_host_project_mean": (_i, [_vp, _i]),
    "hyteg_host_stokes_operator_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_stokes_operator_destroy": (_i, [_vp]),
    "hyteg_host_stokes_operator_apply": (_i, [_vp, _vp, _vp, _i, _i]),
    "hyteg_host_stokes_uzawa_create": (_i, [_vp, _i, _i, _d, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_stokes_gmg_create": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_stokes_gmg_create_with_coarse": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_stokes_minres_create": (_i, [_vp, _i, _i, _i, _d, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_stokes_minres_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_storage_shell_size": (_i, [_i, _ip]),
    "hyteg_host_storage_shell_points": (_i, [_vp, _i, _i, _dp]),
    "hyteg_host_project_normal_create": (_i, [_vp, _i, _i, NORMAL_CB, _vp, C.POINTER(_vp)]),
    "hyteg_host_project_normal_destroy": (_i, [_vp]),
    "hyteg_host_project_normal_project": (_i, [_vp, _vp, _vp, _vp, _i, _i]),
    "hyteg_host_project_normal_project_stokes": (_i, [_vp, _vp, _i, _i]),
    "hyteg_host_stokes_freeslip_wrapper_create": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_stokes_freeslip_wrapper_destroy": (_i, [_vp]),
    "hyteg_host_stokes_freeslip_wrapper_apply": (_i, [_vp, _vp, _vp, _i, _i]),
    "hyteg_host_stokes_freeslip_minres_create": (_i, [_vp, _i, _i, _i, _d, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_stokes_freeslip_minres_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_stokes_freeslip_minres_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_stokes_freeslip_minres_destroy": (_i, [_vp]),
    "hyteg_host_storage_edge_shell_size": (_i, [_i, _ip]),
    "hyteg_host_storage_edge_shell_points": (_i, [_vp, _i, _i, _dp]),
    "hyteg_host_p2_project_normal_create": (_i, [_vp, _i, _i, NORMAL_CB, _vp, C.POINTER(_vp)]),
    "hyteg_host_p2_project_normal_destroy": (_i, [_vp]),
    "hyteg_host_p2_project_normal_project": (_i, [_vp, _vp, _vp, _vp, _i, _i]),
    "hyteg_host_p2_project_normal_project_stokes": (_i, [_vp, _vp, _i, _i]),
    "hyteg_host_th_freeslip_wrapper_create": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_th_freeslip_wrapper_destroy": (_i, [_vp]),
    "hyteg_host_th_freeslip_wrapper_apply": (_i, [_vp, _vp, _vp, _i, _i]),
    "hyteg_host_th_freeslip_minres_create": (_i, [_vp, _i, _i, _i, _d, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_th_freeslip_minres_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_th_freeslip_minres_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_th_freeslip_minres_destroy": (_i, [_vp]),
    "hyteg_host_solver_create_minres": (_i, [_vp, _i, _i, _i, _d, _i, C.POINTER(_vp)]),
    "hyteg_host_stokes_solver_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_stokes_solver_destroy": (_i, [_vp]),
    "hyteg_host_operator_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_operator_destroy": (_i, [_vp]),
    "hyteg_host_operator_stencils": (_i, [_vp, _i, _i, _dp, _dp]),
    "hyteg_host_operator_apply": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "hyteg_host_operator_apply_cycle": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), _i, _i, _i, _i, _i]),
    "hyteg_host_operator_apply_cycle_timed": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), _i, _i, _i, _i, _i, _vp, _vp]),
    "hyteg_host_operator_smooth_jac": (_i, [_vp, _vp, _vp, _vp, _d, _i, _i]),
    "hyteg_host_operator_smooth_sor": (_i, [_vp, _vp, _vp, _d, _i, _i, _i]),
    "hyteg_host_operator_smooth_sor_many": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), _d, _i, _i, _i]),
    "hyteg_host_operator_compute_inverse_diagonal": (_i, [_vp]),
    "hyteg_host_operator_inverse_diagonal": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_elementwise_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_elementwise_destroy": (_i, [_vp]),
    "hyteg_host_elementwise_apply": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "hyteg_host_elementwise_compute_inverse_diagonal": (_i, [_vp]),
    "hyteg_host_elementwise_inverse_diagonal": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_elementwise_smooth_jac": (_i, [_vp, _vp, _vp, _vp, _d, _i, _i]),
    "hyteg_host_divkgrad_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "hyteg_host_divkgrad_destroy": (_i, [_vp]),
    "hyteg_host_divkgrad_apply": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "hyteg_host_divkgrad_compute_inverse_diagonal": (_i, [_vp]),
    "hyteg_host_divkgrad_inverse_diagonal": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_divkgrad_smooth_jac": (_i, [_vp, _vp, _vp, _vp, _d, _i, _i]),
    "hyteg_host_divkgrad_residual": (_i, [_vp, _vp, _vp, _vp, _i, _i]),
    "hyteg_host_divkgrad_set_fused": (_i, [_vp, _i]),
    "hyteg_host_divkgrad_cg_create": (_i, [_vp, _i, _i, _i, _d, _vp, C.POINTER(_vp)]),
    "hyteg_host_divkgrad_cg_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_divkgrad_smoother_create": (_i, [_vp, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_divkgrad_gmg_create": (_i, [_vp, _i, _i, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_divkgrad_chebyshev_estimate_radius": (_i, [_vp, _i, _i, _vp, _vp, C.POINTER(_d)]),
    "hyteg_host_divkgrad_chebyshev_create": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, C.POINTER(_vp)]),
    "hyteg_host_divkgrad_gmg_create_chebyshev": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_divkgrad_solver_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_divkgrad_solver_destroy": (_i, [_vp]),
    "hyteg_host_p2divkgrad_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "hyteg_host_p2divkgrad_destroy": (_i, [_vp]),
    "hyteg_host_p2divkgrad_apply": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "hyteg_host_p2divkgrad_gemv": (_i, [_vp, _d, _vp, _d, _vp, _i, _i]),
    "hyteg_host_p2divkgrad_compute_inverse_diagonal": (_i, [_vp]),
    "hyteg_host_p2divkgrad_inverse_diagonal_copy": (_i, [_vp, _vp, _i]),
    "hyteg_host_p2divkgrad_smooth_jac": (_i, [_vp, _vp, _vp, _vp, _d, _i, _i]),
    "hyteg_host_p2divkgrad_set_fused": (_i, [_vp, _i]),
    "hyteg_host_p2divkgrad_chebyshev_fusable": (_i, [_vp, _i, C.POINTER(_i)]),
    "hyteg_host_p2divkgrad_residual": (_i, [_vp, _vp, _vp, _vp, _i, _i]),
    "hyteg_host_p2divkgrad_cg_create": (_i, [_vp, _i, _i, _i, _d, _vp, C.POINTER(_vp)]),
    "hyteg_host_p2divkgrad_cg_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_p2divkgrad_smoother_create": (_i, [_vp, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2divkgrad_gmg_create": (_i, [_vp, _i, _i, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2divkgrad_chebyshev_estimate_radius": (_i, [_vp, _i, _i, _vp, _vp, C.POINTER(_d)]),
    "hyteg_host_p2divkgrad_chebyshev_create": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, C.POINTER(_vp)]),
    "hyteg_host_p2divkgrad_gmg_create_chebyshev": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2divkgrad_fmg_create": (_i, [_vp, _vp, _i, _i, C.POINTER(C.c_uint), _i, C.POINTER(_vp)]),
    "hyteg_host_p2divkgrad_solver_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_p2divkgrad_solver_destroy": (_i, [_vp]),
    "hyteg_host_p2massoperator_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_p2massoperator_apply": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "hyteg_host_p2massoperator_destroy": (_i, [_vp]),
    "hyteg_host_p2epsilon_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "hyteg_host_p2epsilon_destroy": (_i, [_vp]),
    "hyteg_host_p2epsilon_apply": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _i, _i, _i]),
    "hyteg_host_p2epsilon_gemv": (_i, [_vp, _d, C.POINTER(_vp), _d, C.POINTER(_vp), _i, _i]),
    "hyteg_host_p2epsilon_compute_inverse_diagonal": (_i, [_vp]),
    "hyteg_host_p2epsilon_inverse_diagonal": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_p2epsilon_smooth_jac": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _d, _i, _i]),
    "hyteg_host_p2epsilon_set_fused": (_i, [_vp, _i]),
    "hyteg_host_p2epsilon_chebyshev_fusable": (_i, [_vp, _i, C.POINTER(_i)]),
    "hyteg_host_p2epsilon_residual": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _i, _i]),
    "hyteg_host_p2epsilon_gmg_create": (_i, [_vp, _i, _i, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2epsilon_gmg_create_chebyshev": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2epsilon_cg_create": (_i, [_vp, _i, _i, _i, _d, _vp, C.POINTER(_vp)]),
    "hyteg_host_p2epsilon_cg_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_p2epsilon_smoother_create": (_i, [_vp, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2epsilon_chebyshev_estimate_radius": (_i, [_vp, _i, _i, C.POINTER(_d)]),
    "hyteg_host_p2epsilon_chebyshev_create": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, C.POINTER(_vp)]),
    "hyteg_host_p2epsilon_solver_solve": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _i]),
    "hyteg_host_p2epsilon_solver_destroy": (_i, [_vp]),
    "hyteg_host_th_epsilon_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "hyteg_host_th_epsilon_destroy": (_i, [_vp]),
    "hyteg_host_th_epsilon_apply": (_i, [_vp, _vp, _vp, _i, _i]),
    "hyteg_host_th_epsilon_minres_create": (_i, [_vp, _i, _i, _i, _d, _i, _vp, C.POINTER(_vp)]),
    "hyteg_host_th_epsilon_minres_create_block": (_i, [_vp, _i, _i, _i, _d, _i, _vp, _i, _i, _i, _i, _dp, _i, _d, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_th_epsilon_minres_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_th_epsilon_minres_precondition": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_th_epsilon_minres_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_th_epsilon_minres_destroy": (_i, [_vp]),
    "hyteg_host_epsilon_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "hyteg_host_epsilon_destroy": (_i, [_vp]),
    "hyteg_host_epsilon_apply": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), _i, _i, _i]),
    "hyteg_host_epsilon_compute_inverse_diagonal": (_i, [_vp]),
    "hyteg_host_epsilon_inverse_diagonal": (_i, [_vp, C.POINTER(_vp)]),
    "hyteg_host_epsilon_smooth_jac": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _d, _i, _i]),
    "hyteg_host_epsilon_set_fused": (_i, [_vp, _i]),
    "hyteg_host_epsilon_residual": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _i, _i]),
    "hyteg_host_epsilon_chebyshev_estimate_radius": (_i, [_vp, _i, _i, C.POINTER(_d)]),
    "hyteg_host_epsilon_cg_create": (_i, [_vp, _i, _i, _i, _d, _vp, C.POINTER(_vp)]),
    "hyteg_host_epsilon_cg_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_epsilon_smoother_create": (_i, [_vp, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_epsilon_gmg_create": (_i, [_vp, _i, _i, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_epsilon_chebyshev_create": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, C.POINTER(_vp)]),
    "hyteg_host_epsilon_gmg_create_chebyshev": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_epsilon_solver_solve": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _i]),
    "hyteg_host_epsilon_solver_destroy": (_i, [_vp]),
    "hyteg_host_epsilon_stokes_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "hyteg_host_epsilon_stokes_destroy": (_i, [_vp]),
    "hyteg_host_epsilon_stokes_apply": (_i, [_vp, _vp, _vp, _i, _i]),
    "hyteg_host_epsilon_stokes_minres_create": (_i, [_vp, _i, _i, _i, _d, _i, _vp, C.POINTER(_vp)]),
    "hyteg_host_epsilon_stokes_minres_create_block": (_i, [_vp, _i, _i, _i, _d, _i, _vp, _i, _i, _i, _dp, _i, _d, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_epsilon_stokes_minres_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_epsilon_stokes_minres_precondition": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_epsilon_stokes_minres_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_epsilon_stokes_minres_destroy": (_i, [_vp]),
    "hyteg_host_restrict": (_i, [_vp, _i, _i]),
    "hyteg_host_prolongate": (_i, [_vp, _i, _i]),
    "hyteg_host_prolongate_and_add": (_i, [_vp, _i, _i]),
    "hyteg_host_p1_to_p2": (_i, [_vp, _vp, _i, _i]),
    "hyteg_host_p2_to_p1": (_i, [_vp, _vp, _i, _i]),
    "hyteg_host_quadratic_prolongation_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_quadratic_prolongation_prolongate": (_i, [_vp, _vp, _i, _i]),
    "hyteg_host_quadratic_prolongation_destroy": (_i, [_vp]),
    "hyteg_host_fmg_create": (_i, [_vp, _vp, _i, _i, C.POINTER(_u), _i, _i, LEVEL_CB, _vp, LEVEL_CB, _vp, C.POINTER(_vp)]),
    "hyteg_host_p2_fmg_create": (_i, [_vp, _vp, _i, _i, C.POINTER(_u), _i, LEVEL_CB, _vp, LEVEL_CB, _vp, C.POINTER(_vp)]),
    "hyteg_host_gmg_create": (_i, [_vp, _i, _i, _i, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_chebyshev_coefficients": (_i, [_i, _d, _d, _dp]),
    "hyteg_host_chebyshev_estimate_radius": (_i, [_vp, _i, _i, _vp, _vp, C.POINTER(_d)]),
    "hyteg_host_chebyshev_create": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, C.POINTER(_vp)]),
    "hyteg_host_chebyshev_set_fused": (_i, [_vp, _i]),
    "hyteg_host_gmg_create_chebyshev": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_gmg_set_use_graphs": (_i, [_vp, _i]),
    "hyteg_host_cg_set_use_device_scalars": (_i, [_vp, _i]),
    "hyteg_host_cg_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_gmg_replayed_cycles": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_cg_create": (_i, [_vp, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_cg_create_preconditioned": (_i, [_vp, _i, _i, _i, _d, _vp, C.POINTER(_vp)]),
    "hyteg_host_cg_set_use_fused_update": (_i, [_vp, _i]),
    "hyteg_host_smoother_create": (_i, [_vp, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2_cg_create_preconditioned": (_i, [_vp, _i, _i, _i, _d, _vp, C.POINTER(_vp)]),
    "hyteg_host_p2_cg_iterations": (_i, [_vp, C.POINTER(_i)]),
    "hyteg_host_p2_smoother_create": (_i, [_vp, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_solver_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_solver_solve_steps": (_i, [_vp, _vp, _vp, _vp, _i, _i]),
    "hyteg_host_mixed_precision_jacobi_create": (_i, [_vp, _i, _i, _d, _i, C.POINTER(_vp)]),
    "hyteg_host_solver_destroy": (_i, [_vp]),
    "hyteg_host_p2function_create": (_i, [_vp, C.c_char_p, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_p2function_destroy": (_i, [_vp]),
    "hyteg_host_p2function_pointers": (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_vp)]),
    "hyteg_host_p2function_upload": (_i, [_vp, _i, _i, _vp, _vp]),
    "hyteg_host_p2function_download": (_i, [_vp, _i, _i, _vp, _vp]),
    "hyteg_host_p2function_interpolate_constant": (_i, [_vp, _d, _i, _i]),
    "hyteg_host_p2function_assign": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_vp), _i, _i]),
    "hyteg_host_p2function_add": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_vp), _i, _i]),
    "hyteg_host_p2function_mult_elementwise": (_i, [_vp, _i, C.POINTER(_vp), _i, _i]),
    "hyteg_host_p2_chebyshev_estimate_radius": (_i, [_vp, _i, _i, _vp, _vp, C.POINTER(_d)]),
    "hyteg_host_p2_chebyshev_create": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, C.POINTER(_vp)]),
    "hyteg_host_p2_gmg_create_chebyshev": (_i, [_vp, _i, _i, _i, _dp, _i, _d, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2function_dot": (_i, [_vp, _vp, _i, _i, C.POINTER(_d)]),
    "hyteg_host_p2operator_create_constant": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_p2_prolongate": (_i, [_vp, _i, _i, _i]),
    "hyteg_host_p2_restrict": (_i, [_vp, _i, _i]),
    "hyteg_host_p2operator_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "hyteg_host_p2operator_destroy": (_i, [_vp]),
    "hyteg_host_p2operator_constant_stencils": (_i, [_vp, _i, _i, _dp, _i, C.POINTER(_i)]),
    "hyteg_host_p2operator_element_matrices": (_i, [_vp, _i, _i, _vp]),
    "hyteg_host_p2operator_apply": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "hyteg_host_p2_cg_solve": (_i, [_vp, _vp, _vp, _vp, _i, _i, _d, C.POINTER(_i)]),
    "hyteg_host_p2operator_compute_inverse_diagonal": (_i, [_vp]),
    "hyteg_host_p2operator_inverse_diagonal_copy": (_i, [_vp, _vp, _i]),
    "hyteg_host_p2operator_smooth_jac": (_i, [_vp, _vp, _vp, _vp, _d, _i, _i]),
    "hyteg_host_p2operator_smooth_sor": (_i, [_vp, _vp, _vp, _d, _i, _i, _i]),
    "hyteg_host_p2_gmg_create": (_i, [_vp, _i, _i, _i, _d, _i, _i, _i, _i, _d, C.POINTER(_vp)]),
    "hyteg_host_p2_solver_solve": (_i, [_vp, _vp, _vp, _vp, _i]),
    "hyteg_host_p2_solver_destroy": (_i, [_vp]),
}


class HytegHostError(RuntimeError):
    pass


_lib = None


def lib_path() -> Path:
    return _LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise HytegHostError(f"{_LIB_PATH} not found: run __graft_entry__.build()")
        # libhyteg_host.so depends on libhyteg_hip.so next to it (rpath $ORIGIN)
        l = C.CDLL(str(_LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            f = getattr(l, name)
            f.restype, f.argtypes = res, args
        _lib = l
    return _lib


# an exception raised inside a communication hook (a Python callback called from C++) cannot cross the C frames: the
# trampoline stores it here and returns non-zero, the host layer aborts the operation, and _ck re-raises it
_hook_exception = None


def _ck(rc, what):
    global _hook_exception
    if rc != 0:
        msg = f"{what}: {lib().hyteg_host_last_error().decode(errors='replace')}"
        if _hook_exception is not None:
            exc, _hook_exception = _hook_exception, None
            raise HytegHostError(msg) from exc
        raise HytegHostError(msg)


def _radii(radii):
    r = np.atleast_1d(np.asarray(radii, dtype=np.float64)).copy()
    return r, r.ctypes.data_as(_dp), int(r.size)


def chebyshev_coefficients(order: int, lower: float, upper: float) -> np.ndarray:
    """chebyshev::coefficients: monomial coefficients c[0..order-1] of p in
    1 - l p(l) = T_n((theta - l) / delta) / T_n(theta / delta); needs no GPU"""
    if order < 1:
        raise ValueError("chebyshev_coefficients: order must be at least 1")
    out = np.empty(int(order))
    _ck(lib().hyteg_host_chebyshev_coefficients(int(order), float(lower), float(upper), out.ctypes.data_as(_dp)), "chebyshev_coefficients")
    return out


def estimate_radius(op, level: int, max_iter: int, x, tmp) -> float:
    """chebyshev::estimateRadius: spectral radius of D^-1 A by max_iter power iterations from the start vector x (overwritten);
    op: P1ConstantOperator with P1Functions, or a P2 Laplace operator with P2Functions (inverse diagonal computed)"""
    r = _d()
    fn = lib().hyteg_host_p2_chebyshev_estimate_radius if isinstance(op, P2ElementwiseLaplaceOperator) else lib().hyteg_host_chebyshev_estimate_radius
    if isinstance(op, P1ElementwiseDivKGrad):
        fn = lib().hyteg_host_divkgrad_chebyshev_estimate_radius
    if isinstance(op, P2ElementwiseDivKGrad):
        fn = lib().hyteg_host_p2divkgrad_chebyshev_estimate_radius
    _ck(fn(op.h, int(level), int(max_iter), x.h, tmp.h, C.byref(r)), "chebyshev_estimate_radius")
    return r.value


def cell_size(level: int) -> int:
    n = (1 << level) + 1
    return n * (n + 1) * (n + 2) // 6


class Reduction(NamedTuple):
    """the statistics of a function from one pass over its arrays (P1Function::reduceLocal)"""
    sum: float
    sum_abs: float
    min: float
    max: float
    max_magnitude: float


class _Reductions:
    """sumGlobal / getMaxDoFValue / getMinDoFValue / getMaxDoFMagnitude of the function classes (VertexDoFFunction.cpp:1796-2057,
    P2Function.cpp:351-365, 566-605).  The sums count every DoF once and the cell interiors only if `flag` contains Inner; the
    extrema always include the cell interiors, whatever the flag -- the reference's rule."""

    _reduce_fn = None  # name of the facade function

    def reduce(self, level, flag=All, mpi_reduce=True) -> Reduction:
        out = (C.c_double * 5)()
        _ck(getattr(lib(), self._reduce_fn)(self.h, int(level), int(flag), int(bool(mpi_reduce)), out), self._reduce_fn)
        return Reduction(*out)

    def sum(self, level, flag=All, absolute=False):
        r = self.reduce(level, flag)
        return r.sum_abs if absolute else r.sum

    def max_value(self, level, flag=All, mpi_reduce=True):
        return self.reduce(level, flag, mpi_reduce).max

    def min_value(self, level, flag=All, mpi_reduce=True):
        return self.reduce(level, flag, mpi_reduce).min

    def max_magnitude(self, level, flag=All, mpi_reduce=True):
        return self.reduce(level, flag, mpi_reduce).max_magnitude


class BoundaryUID(NamedTuple):
    """names one boundary of a BoundaryCondition (hyteg::BoundaryUID); id 0: the flags that were given no boundary"""
    id: int
    name: str


class Primitive(NamedTuple):
    """a macro-vertex, -edge or -face: (sorted) global vertex ids, their coordinates, mesh boundary flag, on the domain boundary"""
    vertex_ids: tuple
    coordinates: np.ndarray
    flag: int
    on_boundary: bool


class BoundaryCondition:
    """hyteg::BoundaryCondition: maps the mesh boundary flag of a macro-primitive to a DoFType.  A value: a function that is
    given one keeps a copy."""

    def __init__(self, _handle=None):
        if _handle is None:
            _handle = _vp()
            _ck(lib().hyteg_host_boundary_condition_create(0, C.byref(_handle)), "boundary_condition_create")
        self.h = _handle

    @classmethod
    def _preset(cls, preset):
        h = _vp()
        _ck(lib().hyteg_host_boundary_condition_create(preset, C.byref(h)), "boundary_condition_create")
        return cls(h)

    @classmethod
    def create_0123(cls):
        """1 -> Dirichlet, 2 -> Neumann, 3 -> free slip, every other flag -> Inner"""
        return cls._preset(1)

    @classmethod
    def create_all_inner(cls):
        return cls._preset(2)

    def create_domain(self, name, dof_type, flags) -> BoundaryUID:
        f = [int(flags)] if np.isscalar(flags) else [int(x) for x in flags]
        arr = (_ull * max(len(f), 1))(*f)
        uid = _i()
        _ck(lib().hyteg_host_boundary_condition_create_domain(self.h, name.encode(), int(dof_type), len(f), arr, C.byref(uid)),
            "boundary_condition_create_domain")
        return BoundaryUID(uid.value, name)

    def create_inner(self, name, flags):
        return self.create_domain(name, Inner, flags)

    def create_dirichlet(self, name, flags):
        return self.create_domain(name, DirichletBoundary, flags)

    def create_neumann(self, name, flags):
        return self.create_domain(name, NeumannBoundary, flags)

    def create_freeslip(self, name, flags):
        return self.create_domain(name, FreeslipBoundary, flags)

    def boundary_type(self, flag) -> int:
        t = _i()
        _ck(lib().hyteg_host_boundary_condition_type(self.h, int(flag), C.byref(t)), "boundary_condition_type")
        return t.value

    def boundary_uid(self, flag) -> BoundaryUID:
        """getBoundaryUIDFromMeshFlag"""
        uid = _i()
        buf = C.create_string_buffer(256)
        _ck(lib().hyteg_host_boundary_condition_uid(self.h, int(flag), C.byref(uid), buf, 256), "boundary_condition_uid")
        return BoundaryUID(uid.value, buf.value.decode())

    def __eq__(self, other):
        if not isinstance(other, BoundaryCondition):
            return NotImplemented
        eq = _i()
        _ck(lib().hyteg_host_boundary_condition_equal(self.h, other.h, C.byref(eq)), "boundary_condition_equal")
        return bool(eq.value)

    __hash__ = None

    def close(self):
        if self.h:
            lib().hyteg_host_boundary_condition_destroy(self.h)
        self.h = None

    def __del__(self):  # a value object handed out freely (Function.boundary_condition makes a copy per access): freed with it
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown: the library may be gone
            pass


class _BoundaryConditioned:
    """set_boundary_condition / boundary_condition / interpolate on one boundary, for P1Function and P2Function"""

    _bc_prefix = None  # "hyteg_host_function" or "hyteg_host_p2function"

    def set_boundary_condition(self, bc: BoundaryCondition):
        """Function::setBoundaryCondition: the function keeps a copy"""
        _ck(getattr(lib(), self._bc_prefix + "_set_boundary_condition")(self.h, bc.h), "set_boundary_condition")

    @property
    def boundary_condition(self) -> BoundaryCondition:
        """a copy of the function's condition (the storage's default one if it was given none)"""
        h = _vp()
        _ck(getattr(lib(), self._bc_prefix + "_boundary_condition")(self.h, C.byref(h)), "boundary_condition")
        return BoundaryCondition(h)

    def _interpolate_on_boundary(self, value, level, boundary_uid: BoundaryUID):
        """a BoundaryUID belongs to the condition that created it: one that is not a boundary of this function's condition fails"""
        _ck(getattr(lib(), self._bc_prefix + "_interpolate_constant_on_boundary")(self.h, float(value), level, int(boundary_uid.id),
                                                                                  boundary_uid.name.encode()), "interpolate (boundary)")


class Storage:
    """hyteg::PrimitiveStorage"""

    def __init__(self, handle):
        self.h = handle
        self._hooks = None
        self.stream = 0  # raw hipStream_t the host layer launches on (0: the null stream)
        c = (C.c_int * 6)()
        _ck(lib().hyteg_host_storage_counts(self.h, c), "storage_counts")
        self.n_cells, self.n_faces, self.n_edges, self.n_vertices, self.n_local_cells, self.n_ranks = list(c)

    @classmethod
    def from_gmsh(cls, path, rank=0, nranks=1):
        h = _vp()
        _ck(lib().hyteg_host_storage_from_gmsh(str(path).encode(), rank, nranks, C.byref(h)), "storage_from_gmsh")
        return cls(h)

    @classmethod
    def from_arrays(cls, vertices, cells, rank=0, nranks=1):
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 4)
        h = _vp()
        _ck(lib().hyteg_host_storage_from_arrays(len(v), v.ctypes.data_as(_dp), len(c), c.ctypes.data_as(_ip), rank, nranks,
                                                 C.byref(h)), "storage_from_arrays")
        return cls(h)

    @classmethod
    def single_tet(cls, coords):
        return cls.from_arrays(coords, [[0, 1, 2, 3]])

    def local_cell(self, i):
        gid = C.c_int()
        co = np.empty(12)
        nnc = np.empty(14)
        _ck(lib().hyteg_host_storage_local_cell(self.h, i, C.byref(gid), co.ctypes.data_as(_dp), nnc.ctypes.data_as(_dp)),
            "storage_local_cell")
        return gid.value, co.reshape(4, 3), nnc

    def shell_points(self, i, level):
        """(shell size, 3): the coordinates, in the order of the shell enumeration (capi.p1_shell_enumeration), at which a
        P1ProjectNormalOperator evaluates its normal function in local cell i: the vertex DoFs on the macro-faces with one neighbour
        cell and on their edges and vertices.  NaN at every other entry.  Host only."""
        n = _i()
        _ck(lib().hyteg_host_storage_shell_size(int(level), C.byref(n)), "storage_shell_size")
        out = np.empty((n.value, 3))
        _ck(lib().hyteg_host_storage_shell_points(self.h, int(i), int(level), out.ctypes.data_as(_dp)), "storage_shell_points")
        return out

    def edge_shell_points(self, i, level):
        """shell_points for the edge DoFs of a P2ProjectNormalOperator: (edge shell size, 3) midpoints of the micro-edges on the
        boundary primitives of local cell i, in the order of capi.p2_edge_shell_enumeration; NaN elsewhere.  Host only."""
        n = _i()
        _ck(lib().hyteg_host_storage_edge_shell_size(int(level), C.byref(n)), "storage_edge_shell_size")
        out = np.empty((n.value, 3))
        _ck(lib().hyteg_host_storage_edge_shell_points(self.h, int(i), int(level), out.ctypes.data_as(_dp)), "storage_edge_shell_points")
        return out

    def mask(self, i, flag, owned=False, bc=None):
        """point mask of local cell i under `flag`; bc: a BoundaryCondition (None: the storage's default one)"""
        m = _u()
        if bc is None:
            _ck(lib().hyteg_host_storage_mask(self.h, i, flag, int(owned), C.byref(m)), "storage_mask")
        else:
            _ck(lib().hyteg_host_storage_mask_bc(self.h, i, flag, int(owned), bc.h, C.byref(m)), "storage_mask")
        return m.value

    # ---- mesh boundary flags (SetupPrimitiveStorage::setMeshBoundaryFlags*): before the first function, operator or plan ----
    def set_mesh_boundary_flags_on_boundary(self, flag_on_boundary, flag_inner, highest_dimension_always_inner=True):
        _ck(lib().hyteg_host_storage_set_mesh_boundary_flags_on_boundary(self.h, int(flag_on_boundary), int(flag_inner),
                                                                        int(bool(highest_dimension_always_inner))),
            "set_mesh_boundary_flags_on_boundary")

    def set_mesh_boundary_flags_inner(self, flag_inner, highest_dimension_always_inner=True):
        _ck(lib().hyteg_host_storage_set_mesh_boundary_flags_inner(self.h, int(flag_inner), int(bool(highest_dimension_always_inner))),
            "set_mesh_boundary_flags_inner")

    @staticmethod
    def _location_callback(predicate):
        def call(user, xyz):
            global _hook_exception
            try:
                return 1 if predicate(xyz[0], xyz[1], xyz[2]) else 0
            except BaseException as e:  # noqa: BLE001 - must not propagate into the C frames
                if _hook_exception is None:
                    _hook_exception = e
                return 0
        return LOCATION_CB(call)

    @staticmethod
    def _ck_location(rc, what):
        global _hook_exception
        _ck(rc, what)
        if _hook_exception is not None:
            exc, _hook_exception = _hook_exception, None
            raise HytegHostError(f"{what}: the predicate raised") from exc

    def set_mesh_boundary_flags_by_vertex_location(self, flag, predicate, all_vertices=True):
        """flag on every primitive whose vertices all (all_vertices=False: at least one) satisfy predicate(x, y, z)"""
        cb = self._location_callback(predicate)
        self._ck_location(lib().hyteg_host_storage_set_mesh_boundary_flags_by_vertex_location(self.h, int(flag), cb, None,
                                                                                              int(bool(all_vertices))),
                          "set_mesh_boundary_flags_by_vertex_location")

    def set_mesh_boundary_flags_by_centroid_location(self, flag, predicate):
        """flag on every primitive whose centroid satisfies predicate(x, y, z)"""
        cb = self._location_callback(predicate)
        self._ck_location(lib().hyteg_host_storage_set_mesh_boundary_flags_by_centroid_location(self.h, int(flag), cb, None),
                          "set_mesh_boundary_flags_by_centroid_location")

    def set_mesh_boundary_flag(self, dim, index, flag):
        """dim 0: macro-vertex, 1: -edge, 2: -face"""
        _ck(lib().hyteg_host_storage_set_mesh_boundary_flag(self.h, int(dim), int(index), int(flag)), "set_mesh_boundary_flag")

    def primitive(self, dim, index) -> Primitive:
        n, ids, co, flag, onb = _i(), (C.c_int * 3)(), np.zeros(9), _ull(), _i()
        _ck(lib().hyteg_host_storage_primitive(self.h, int(dim), int(index), C.byref(n), ids, co.ctypes.data_as(_dp), C.byref(flag),
                                               C.byref(onb)), "storage_primitive")
        return Primitive(tuple(ids[:n.value]), co.reshape(3, 3)[:n.value].copy(), flag.value, bool(onb.value))

    def n_primitives(self, dim):
        return (self.n_vertices, self.n_edges, self.n_faces)[dim]

    @property
    def boundary_classes(self):
        """the mesh flags of the exchange classes, ascending: class c has the plans of key (c & 1) + 2 * dof_kind + 4 * (c >> 1).
        Asking fixes the mesh boundary flags."""
        n = _i()
        _ck(lib().hyteg_host_storage_boundary_classes(self.h, C.byref(n), None), "boundary_classes")
        f = (_ull * max(n.value, 1))()
        _ck(lib().hyteg_host_storage_boundary_classes(self.h, C.byref(n), f), "boundary_classes")
        return [int(x) for x in f[:n.value]]

    @staticmethod
    def plan_key(cls, dof_kind=0):
        return (cls & 1) + 2 * dof_kind + 4 * (cls >> 1)

    @property
    def default_boundary_condition(self) -> BoundaryCondition:
        h = _vp()
        _ck(lib().hyteg_host_storage_default_boundary_condition(self.h, C.byref(h)), "default_boundary_condition")
        return BoundaryCondition(h)

    def set_boundary_type(self, t):
        _ck(lib().hyteg_host_storage_set_boundary_type(self.h, t), "set_boundary_type")

    def set_batch_max_level(self, level):
        """levels <= level run the batched kernels (one launch for all local cells); -1: per-cell kernels everywhere"""
        _ck(lib().hyteg_host_storage_set_batch_max_level(self.h, level), "set_batch_max_level")

    def set_apply_steps(self, steps):
        """steps per launch of apply_cycle on one macro-cell (independent consecutive applies share a launch); 1: one launch per
        apply, 0: default (HYTEG_AMD_APPLY_STEPS, else 16)"""
        _ck(lib().hyteg_host_storage_set_apply_steps(self.h, steps), "set_apply_steps")

    def set_apply_lanes(self, lanes):
        """stream lanes for independent interior launches inside one host-layer call (apply_cycle); 1: one stream, 0: default
        (HYTEG_AMD_APPLY_LANES, else 2)"""
        _ck(lib().hyteg_host_storage_set_apply_lanes(self.h, lanes), "set_apply_lanes")

    def set_apply_cell_lanes_min(self, cells):
        """multi-cell P1 apply: the cells' interior kernels alternate between the lanes from `cells` local cells on; 0: never"""
        _ck(lib().hyteg_host_storage_set_apply_cell_lanes_min(self.h, cells), "set_apply_cell_lanes_min")

    def lanes_seen(self):
        """bit l: lane l carried a launch in the storage's last lane scope (0: its lanes were off)"""
        m = C.c_uint()
        _ck(lib().hyteg_host_storage_lanes_seen(self.h, C.byref(m)), "lanes_seen")
        return m.value

    def steps_launches(self):
        """launches of more than one step that the storage's last apply_cycle issued (0: it ran as single launches)"""
        n = C.c_uint()
        _ck(lib().hyteg_host_storage_steps_launches(self.h, C.byref(n)), "steps_launches")
        return n.value

    def set_stream(self, stream):
        _ck(lib().hyteg_host_storage_set_stream(self.h, stream), "set_stream")
        self.stream = int(stream) if stream else 0

    def set_hooks(self, exchange_begin, exchange_end, allreduce_sum):
        """hooks(level, key) with key = Storage.plan_key(cls, dof_kind); an exception in a hook fails the operation that called it"""

        def guard(fn):
            def call(user, *args):
                global _hook_exception
                try:
                    fn(*args)
                    return 0
                except BaseException as e:  # noqa: BLE001 - must not propagate into the C frames
                    _hook_exception = e
                    return 1
            return call

        exb, exe, ar = EXCHANGE_CB(guard(exchange_begin)), EXCHANGE_CB(guard(exchange_end)), ALLREDUCE_CB(guard(allreduce_sum))
        self._hooks = (exb, exe, ar)  # keep alive
        _ck(lib().hyteg_host_storage_set_hooks(self.h, exb, exe, ar, None), "set_hooks")

    def use_rccl(self, unique_id: bytes):
        """RCCL over xGMI issued from the C++ host layer (collective over all ranks; the rank's device must be current).
        unique_id: the bytes of capi.comm_unique_id() from rank 0, distributed by the caller."""
        if len(unique_id) != 128:
            raise ValueError("use_rccl: the unique id has 128 bytes")
        _ck(lib().hyteg_host_storage_use_rccl(self.h, bytes(unique_id)), "storage_use_rccl")

    # ---- peer-to-peer transport on top of the current one (see include/hyteg_host.h for the set-up sequence) ----
    def use_p2p(self, arena_bytes: int):
        """-> (this rank's arena handle: 64 bytes, arena kind 0 uncached / 1 fine-grained / 2 default)"""
        buf = C.create_string_buffer(64)
        kind = C.c_int(0)
        _ck(lib().hyteg_host_storage_use_p2p(self.h, int(arena_bytes), buf, C.byref(kind)), "storage_use_p2p")
        return buf.raw, kind.value

    def p2p_open(self, handles):
        """handles: the 64-byte handles of all ranks, rank by rank"""
        blob = b"".join(bytes(h) for h in handles)
        _ck(lib().hyteg_host_storage_p2p_open(self.h, blob), "storage_p2p_open")

    def p2p_layout(self, level: int, key: int, npeers: int):
        """-> int64 array [npeers, 3]: byte offsets (slot 0, slot 1, flag) in this rank's arena of every peer's segment"""
        o = np.zeros((max(npeers, 1), 3), dtype=np.int64)
        _ck(lib().hyteg_host_storage_p2p_layout(self.h, level, key, o.ctypes.data_as(C.POINTER(C.c_longlong))), "storage_p2p_layout")
        return o[:npeers]

    def p2p_connect(self, level: int, key: int, offsets):
        o = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1, 3)
        o = o if len(o) else np.zeros((1, 3), dtype=np.int64)
        _ck(lib().hyteg_host_storage_p2p_connect(self.h, level, key, o.ctypes.data_as(C.POINTER(C.c_longlong))), "storage_p2p_connect")

    def drop_p2p(self):
        _ck(lib().hyteg_host_storage_drop_p2p(self.h), "storage_drop_p2p")

    def check_transport(self):
        """synchronises; raises if a device-side wait of the transport has timed out since the last check"""
        _ck(lib().hyteg_host_storage_check_transport(self.h), "storage_check_transport")

    def allreduce_sum(self, values):
        """sum over all ranks of a sequence of floats (through the storage's transport)"""
        a = np.ascontiguousarray(values, dtype=np.float64).copy()
        _ck(lib().hyteg_host_storage_allreduce_sum(self.h, a.ctypes.data_as(_dp), len(a)), "storage_allreduce_sum")
        return a

    def allreduce_max(self, values):
        """maximum over all ranks of each of a sequence of floats (exact; built on the transport's sum); min = -allreduce_max(-x)"""
        a = np.ascontiguousarray(values, dtype=np.float64).copy()
        _ck(lib().hyteg_host_storage_allreduce_max(self.h, a.ctypes.data_as(_dp), len(a)), "storage_allreduce_max")
        return a

    def number_of_dofs(self, level, p2=False, global_=True):
        """numberOfGlobalDoFs / numberOfLocalDoFs of a P1 (p2: a P2) function: what the sum of a function of ones gives"""
        n = C.c_ulonglong()
        fn = lib().hyteg_host_storage_p2_number_of_dofs if p2 else lib().hyteg_host_storage_p1_number_of_dofs
        _ck(fn(self.h, int(level), int(bool(global_)), C.byref(n)), "number_of_dofs")
        return n.value

    def enable_timing(self, on=True, synchronize=False):
        """walberla-style timing tree with the reference's timer names; synchronize: ranges measure device execution"""
        _ck(lib().hyteg_host_storage_enable_timing(self.h, int(on), int(synchronize)), "storage_enable_timing")

    def timing_json(self) -> str:
        """the tree in the layout of walberla::timing::to_json (hyteg::writeTimingTreeJSON)"""
        need = C.c_size_t()
        _ck(lib().hyteg_host_storage_timing_json(self.h, None, 0, C.byref(need)), "storage_timing_json")
        buf = C.create_string_buffer(need.value)
        _ck(lib().hyteg_host_storage_timing_json(self.h, buf, need.value, None), "storage_timing_json")
        return buf.value.decode()

    def timing_reset(self):
        _ck(lib().hyteg_host_storage_timing_reset(self.h), "storage_timing_reset")

    @property
    def transport(self) -> str:
        buf = C.create_string_buffer(32)
        _ck(lib().hyteg_host_storage_transport_name(self.h, buf, 32), "storage_transport_name")
        return buf.value.decode()

    def plan(self, level, key):
        """exchange plan of (level, key = Storage.plan_key(cls, dof_kind)): cls + 2 * dof_kind for the classes 0 and 1"""
        cls = key
        s = (C.c_int * 5)()
        _ck(lib().hyteg_host_plan_sizes(self.h, level, cls, s), "plan_sizes")
        ng, ne, npeer, ts, tr = list(s)
        a = lambda n: np.zeros(max(n, 1), dtype=np.int32)  # noqa: E731
        gp, eb, eo, peers, sc, rc, sb, so = a(ng + 1), a(ne), a(ne), a(npeer), a(npeer), a(npeer), a(ts), a(ts)
        p = lambda x: x.ctypes.data_as(_ip)  # noqa: E731
        _ck(lib().hyteg_host_plan_export(self.h, level, cls, p(gp), p(eb), p(eo), p(peers), p(sc), p(rc), p(sb), p(so)),
            "plan_export")
        return dict(ngroups=ng, group_ptr=gp[:ng + 1], entry_buf=eb[:ne], entry_off=eo[:ne], peers=peers[:npeer],
                    send_count=sc[:npeer], recv_count=rc[:npeer], send_buf=sb[:ts], send_off=so[:ts], total_send=ts,
                    total_recv=tr)

    def register_comm_buffers(self, level, cls, send_ptr, recv_ptr):
        _ck(lib().hyteg_host_plan_register_buffers(self.h, level, cls, send_ptr, recv_ptr), "plan_register_buffers")

    def close(self):
        if self.h:
            lib().hyteg_host_storage_destroy(self.h)
            self.h = None


class P1Function(_Reductions, _BoundaryConditioned):
    """hyteg::P1Function<double>"""
    _reduce_fn = "hyteg_host_p1_reduce"
    _bc_prefix = "hyteg_host_function"

    def __init__(self, storage: Storage, name: str, min_level: int, max_level: int, _borrowed=None):
        self.storage, self.min_level, self.max_level = storage, min_level, max_level
        self._borrowed = _borrowed is not None
        if _borrowed is not None:
            self.h = _borrowed
        else:
            h = _vp()
            _ck(lib().hyteg_host_function_create(storage.h, name.encode(), min_level, max_level, C.byref(h)), "function_create")
            self.h = h

    def cell_pointer(self, c, level):
        p = _vp()
        _ck(lib().hyteg_host_function_cell_pointer(self.h, c, level, C.byref(p)), "cell_pointer")
        return p.value

    def upload_cell(self, c, level, arr):
        a = np.ascontiguousarray(arr, dtype=np.float64)
        assert a.size == cell_size(level)
        _ck(lib().hyteg_host_function_upload_cell(self.h, c, level, a.ctypes.data_as(_dp)), "upload_cell")

    def download_cell(self, c, level):
        a = np.empty(cell_size(level))
        _ck(lib().hyteg_host_function_download_cell(self.h, c, level, a.ctypes.data_as(_dp)), "download_cell")
        return a

    def interpolate(self, value, level, flag=All, boundary_uid=None):
        """boundary_uid: on the primitives whose mesh flag belongs to that boundary of the function's condition (flag is not used)"""
        if boundary_uid is not None:
            return self._interpolate_on_boundary(value, level, boundary_uid)
        _ck(lib().hyteg_host_function_interpolate_constant(self.h, float(value), level, flag), "interpolate")

    def _vec(self, fn, scalars, funcs, level, flag):
        n = len(funcs)
        hs = (_vp * n)(*[f.h for f in funcs])
        if scalars is None:
            _ck(fn(self.h, n, hs, level, flag), "vector op")
        else:
            sc = (C.c_double * n)(*[float(s) for s in scalars])
            _ck(fn(self.h, n, sc, hs, level, flag), "vector op")

    def assign(self, scalars, funcs, level, flag=All):
        self._vec(lib().hyteg_host_function_assign, scalars, funcs, level, flag)

    def add(self, scalars, funcs, level, flag=All):
        self._vec(lib().hyteg_host_function_add, scalars, funcs, level, flag)

    def mult_elementwise(self, funcs, level, flag=All):
        self._vec(lib().hyteg_host_function_mult_elementwise, None, funcs, level, flag)

    def dot(self, other, level, flag=All, global_=True):
        r = C.c_double()
        _ck(lib().hyteg_host_function_dot(self.h, other.h, level, flag, int(global_), C.byref(r)), "dot")
        return r.value

    def sum_shared(self, level, flag=All):
        _ck(lib().hyteg_host_function_sum_shared(self.h, level, flag), "sum_shared")

    def sync_shared(self, level, flag=All):
        _ck(lib().hyteg_host_function_sync_shared(self.h, level, flag), "sync_shared")

    def set_all_inner(self, on=True):
        """BoundaryCondition::createAllInnerBC(): every point of this function counts as Inner (Stokes pressure)"""
        _ck(lib().hyteg_host_function_set_all_inner(self.h, int(on)), "function_set_all_inner")

    def close(self):
        if self.h and not self._borrowed:
            lib().hyteg_host_function_destroy(self.h)
        self.h = None


FORM_LAPLACE, FORM_MASS, FORM_DIV_X, FORM_DIV_Y, FORM_DIV_Z, FORM_DIVT_X, FORM_DIVT_Y, FORM_DIVT_Z, FORM_PSPG = range(9)


class P1ConstantOperator:
    """hyteg::P1ConstantOperator< Form >: form = FORM_LAPLACE (P1ConstantLaplaceOperator), FORM_MASS, FORM_DIV_X/Y/Z
    (P1Div{x,y,z}Operator), FORM_DIVT_X/Y/Z, FORM_PSPG"""

    def __init__(self, storage: Storage, min_level: int, max_level: int, form: int = 0):
        self.storage = storage
        h = _vp()
        _ck(lib().hyteg_host_operator_create(storage.h, min_level, max_level, form, C.byref(h)), "operator_create")
        self.h = h

    def stencils(self, global_cell, level):
        inner, slots = np.empty(15), np.empty(210)
        _ck(lib().hyteg_host_operator_stencils(self.h, global_cell, level, inner.ctypes.data_as(_dp), slots.ctypes.data_as(_dp)),
            "operator_stencils")
        return inner, slots.reshape(14, 15)

    def apply(self, src, dst, level, flag, update=Replace):
        _ck(lib().hyteg_host_operator_apply(self.h, src.h, dst.h, level, flag, update), "apply")

    def apply_cycle(self, srcs, dsts, level, flag, update=Replace, first=0, steps=1):
        """`steps` applies, step k on pair (first + k) % len(srcs): the loop a C++ application writes around apply()"""
        self.prepared_cycle(srcs, dsts, level, flag, update)(first, steps)

    def prepared_cycle(self, srcs, dsts, level, flag, update=Replace):
        """apply_cycle with the handle arrays built once: returns call(first, steps, ev_start=None, ev_stop=None); the two
        optional timing events of the C-ABI (capi.event_create_timing) are recorded on the storage's stream directly before
        the first and after the last apply"""
        n = len(srcs)
        hs, hd = (_vp * n)(*[f.h for f in srcs]), (_vp * n)(*[f.h for f in dsts])
        fn, fnt, h = lib().hyteg_host_operator_apply_cycle, lib().hyteg_host_operator_apply_cycle_timed, self.h

        def call(first, steps, ev_start=None, ev_stop=None):
            if ev_start is None and ev_stop is None:
                _ck(fn(h, n, hs, hd, level, flag, update, first, steps), "apply_cycle")
            else:
                _ck(fnt(h, n, hs, hd, level, flag, update, first, steps, ev_start, ev_stop), "apply_cycle_timed")

        return call

    def smooth_jac(self, dst, rhs, src, relax, level, flag):
        _ck(lib().hyteg_host_operator_smooth_jac(self.h, dst.h, rhs.h, src.h, float(relax), level, flag), "smooth_jac")

    def smooth_sor(self, dst, rhs, relax, level, flag, backwards=False):
        _ck(lib().hyteg_host_operator_smooth_sor(self.h, dst.h, rhs.h, float(relax), level, flag, int(backwards)), "smooth_sor")

    def smooth_sor_many(self, dsts, rhss, relax, level, flag, backwards=False):
        """one sweep of several functions by shared launches (the velocity components of the Stokes smoother)"""
        n = len(dsts)
        hd, hr = (_vp * n)(*[f.h for f in dsts]), (_vp * n)(*[f.h for f in rhss])
        _ck(lib().hyteg_host_operator_smooth_sor_many(self.h, n, hd, hr, float(relax), level, flag, int(backwards)), "smooth_sor_many")

    def smooth_gs(self, dst, rhs, level, flag):
        self.smooth_sor(dst, rhs, 1.0, level, flag)

    def compute_inverse_diagonal(self):
        _ck(lib().hyteg_host_operator_compute_inverse_diagonal(self.h), "computeInverseDiagonalOperatorValues")

    def inverse_diagonal(self, min_level, max_level):
        h = _vp()
        _ck(lib().hyteg_host_operator_inverse_diagonal(self.h, C.byref(h)), "getInverseDiagonalValues")
        return P1Function(self.storage, "invdiag", min_level, max_level, _borrowed=h)

    def close(self):
        if self.h:
            lib().hyteg_host_operator_destroy(self.h)
            self.h = None


class P1ElementwiseDiffusion:
    """hyteg::operatorgeneration::P1ElementwiseDiffusion (the class the hyteg_operators generator emits): every apply goes
    through the C-ABI seam hyteg_hip_p1_elementwise_diffusion_apply_macro_3d_masked with the cell's coordinates"""

    def __init__(self, storage: Storage, min_level: int, max_level: int):
        self.storage = storage
        self.min_level, self.max_level = min_level, max_level
        h = _vp()
        _ck(lib().hyteg_host_elementwise_create(storage.h, min_level, max_level, C.byref(h)), "elementwise_create")
        self.h = h

    def apply(self, src, dst, level, flag, update=Replace):
        _ck(lib().hyteg_host_elementwise_apply(self.h, src.h, dst.h, level, flag, update), "elementwise apply")

    def compute_inverse_diagonal(self):
        _ck(lib().hyteg_host_elementwise_compute_inverse_diagonal(self.h), "computeInverseDiagonalOperatorValues")

    def inverse_diagonal(self):
        h = _vp()
        _ck(lib().hyteg_host_elementwise_inverse_diagonal(self.h, C.byref(h)), "getInverseDiagonalValues")
        return P1Function(self.storage, "invdiag", self.min_level, self.max_level, _borrowed=h)

    def smooth_jac(self, dst, rhs, src, relax, level, flag):
        _ck(lib().hyteg_host_elementwise_smooth_jac(self.h, dst.h, rhs.h, src.h, float(relax), level, flag), "elementwise smooth_jac")

    def close(self):
        if self.h:
            lib().hyteg_host_elementwise_destroy(self.h)
            self.h = None


class P1ElementwiseDivKGrad:
    """hyteg::operatorgeneration::P1ElementwiseDivKGrad( storage, minLevel, maxLevel, k ): -div( k grad u ) with the P1 coefficient
    function k, which holds values on every level min_level..max_level (the operator at level l reads k at level l; levels 0..8).
    Every apply goes through the C-ABI seam hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked."""

    def __init__(self, storage: Storage, min_level: int, max_level: int, k: "P1Function"):
        self.storage = storage
        self.min_level, self.max_level = min_level, max_level
        self.k = k  # the operator reads k on every apply: k outlives it
        h = _vp()
        _ck(lib().hyteg_host_divkgrad_create(storage.h, min_level, max_level, k.h, C.byref(h)), "divkgrad_create")
        self.h = h

    def apply(self, src, dst, level, flag, update=Replace):
        _ck(lib().hyteg_host_divkgrad_apply(self.h, src.h, dst.h, level, flag, update), "divkgrad apply")

    def compute_inverse_diagonal_operator_values(self):
        _ck(lib().hyteg_host_divkgrad_compute_inverse_diagonal(self.h), "computeInverseDiagonalOperatorValues")

    def inverse_diagonal(self):
        h = _vp()
        _ck(lib().hyteg_host_divkgrad_inverse_diagonal(self.h, C.byref(h)), "getInverseDiagonalValues")
        return P1Function(self.storage, "invdiag", self.min_level, self.max_level, _borrowed=h)

    def smooth_jac(self, dst, rhs, src, relax, level, flag):
        _ck(lib().hyteg_host_divkgrad_smooth_jac(self.h, dst.h, rhs.h, src.h, float(relax), level, flag), "divkgrad smooth_jac")

    def residual(self, x, b, r, level, flag):
        """r = b - A x as a multigrid cycle forms it: one fused launch on the inner points, or apply + assign with set_fused(False)"""
        _ck(lib().hyteg_host_divkgrad_residual(self.h, x.h, b.h, r.h, level, flag), "divkgrad residual")

    def set_fused(self, on: bool):
        """smooth_jac, residual and the steps of the Chebyshev smoother: the fused launches on the inner points (default) or the
        composed passes everywhere"""
        _ck(lib().hyteg_host_divkgrad_set_fused(self.h, int(bool(on))), "divkgrad set_fused")

    def close(self):
        if self.h:
            lib().hyteg_host_divkgrad_destroy(self.h)
            self.h = None


class DivKGradSolver:
    """The solvers instantiated for P1ElementwiseDivKGrad: CGSolver, GeometricMultigridSolver (linear P1 transfer, CG on the coarsest
    level) with a weighted-Jacobi or a Chebyshev smoother, and the smoothers on their own.  Built by the class methods."""

    def __init__(self, storage, h, keep=None):
        self.storage, self.h, self._keep = storage, h, keep

    @classmethod
    def cg(cls, storage, min_level, max_level, max_iter=1000, tol=1e-14, preconditioner=None):
        """hyteg::CGSolver< P1ElementwiseDivKGrad >; preconditioner: a DivKGradSolver or None"""
        h = _vp()
        _ck(lib().hyteg_host_divkgrad_cg_create(storage.h, min_level, max_level, max_iter, float(tol),
                                                preconditioner.h if preconditioner is not None else None, C.byref(h)), "divkgrad cg_create")
        return cls(storage, h, preconditioner)

    @classmethod
    def gmg(cls, storage, min_level, max_level, smoother=JACOBI, relax=2.0 / 3.0, pre=3, post=3, wcycle=False, cg_max_iter=1000, cg_tol=1e-14):
        """hyteg::GeometricMultigridSolver with WeightedJacobiSmoother( relax ) (the operator has no Gauss-Seidel sweep)"""
        if smoother != JACOBI:
            raise HytegHostError("DivKGradSolver.gmg: smoother JACOBI (gmg_chebyshev for the Chebyshev smoother)")
        h = _vp()
        _ck(lib().hyteg_host_divkgrad_gmg_create(storage.h, min_level, max_level, float(relax), pre, post, int(bool(wcycle)), cg_max_iter,
                                                 float(cg_tol), C.byref(h)), "divkgrad gmg_create")
        return cls(storage, h)

    @classmethod
    def chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3):
        """hyteg::ChebyshevSmoother< P1ElementwiseDivKGrad > on its own (solve = one smoother call)"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_divkgrad_chebyshev_create(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower),
                                                       C.byref(h)), "divkgrad chebyshev_create")
        return cls(storage, h)

    @classmethod
    def gmg_chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3, pre=1, post=1, wcycle=False, cg_max_iter=1000,
                      cg_tol=1e-14):
        """the multigrid solver smoothing with ChebyshevSmoother( order ); radii: one spectral radius (estimate_radius) or one per level"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_divkgrad_gmg_create_chebyshev(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower), pre,
                                                           post, int(bool(wcycle)), cg_max_iter, float(cg_tol), C.byref(h)),
            "divkgrad gmg_create_chebyshev")
        return cls(storage, h)

    @classmethod
    def smoother(cls, storage, min_level, max_level, smoother=JACOBI, relax=1.0):
        """WeightedJacobiSmoother( relax ) (JACOBI) or IdentityPreconditioner (IDENTITY) on its own"""
        h = _vp()
        _ck(lib().hyteg_host_divkgrad_smoother_create(storage.h, min_level, max_level, {JACOBI: 0, IDENTITY: -1}[smoother], float(relax),
                                                      C.byref(h)), "divkgrad smoother_create")
        return cls(storage, h)

    @property
    def iterations(self) -> int:
        """CGSolver::getIterations of the last solve (DivKGradSolver.cg)"""
        n = _i(0)
        _ck(lib().hyteg_host_divkgrad_cg_iterations(self.h, C.byref(n)), "divkgrad cg_iterations")
        return n.value

    def solve(self, op: P1ElementwiseDivKGrad, x: "P1Function", b: "P1Function", level):
        _ck(lib().hyteg_host_divkgrad_solver_solve(self.h, op.h, x.h, b.h, level), "divkgrad solve")

    def close(self):
        if self.h:
            lib().hyteg_host_divkgrad_solver_destroy(self.h)
            self.h = None


def restrict(f: P1Function, source_level, flag):
    _ck(lib().hyteg_host_restrict(f.h, source_level, flag), "restrict")


def prolongate(f: P1Function, source_level, flag):
    _ck(lib().hyteg_host_prolongate(f.h, source_level, flag), "prolongate")


def prolongate_and_add(f: P1Function, source_level, flag):
    _ck(lib().hyteg_host_prolongate_and_add(f.h, source_level, flag), "prolongateAndAdd")


def p1_to_p2(p1: P1Function, p2: "P2Function", p2_level, flag=All):
    """hyteg::P1toP2Conversion: the P2 function of level p2_level := the P1 function of level p2_level + 1 (a copy, DoF by DoF)"""
    _ck(lib().hyteg_host_p1_to_p2(p1.h, p2.h, p2_level, flag), "P1toP2Conversion")


def p2_to_p1(p2: "P2Function", p1: P1Function, p1_level, flag=All):
    """hyteg::P2toP1Conversion: the P1 function of level p1_level := the P2 function of level p1_level - 1"""
    _ck(lib().hyteg_host_p2_to_p1(p2.h, p1.h, p1_level, flag), "P2toP1Conversion")


class P1QuadraticProlongation:
    """hyteg::P1toP1QuadraticProlongationThroughP2Injection( storage, p1_min_level, p1_max_level ): owns the P2 temporary"""

    def __init__(self, storage: Storage, p1_min_level: int, p1_max_level: int):
        self.storage = storage
        h = _vp()
        _ck(lib().hyteg_host_quadratic_prolongation_create(storage.h, p1_min_level, p1_max_level, C.byref(h)), "P1QuadraticProlongation")
        self.h = h

    def prolongate(self, f: P1Function, source_level, flag):
        _ck(lib().hyteg_host_quadratic_prolongation_prolongate(self.h, f.h, source_level, flag), "prolongate_quadratic")

    def close(self):
        if self.h:
            lib().hyteg_host_quadratic_prolongation_destroy(self.h)
            self.h = None


def prolongate_quadratic(f: P1Function, source_level, flag):
    """One quadratic prolongation source_level -> source_level + 1 with a temporary of its own.  The DoFs of the finer level that
    `flag` excludes end as zero (see hyteg_host.h); a solver that prolongates repeatedly keeps a P1QuadraticProlongation instead."""
    p = P1QuadraticProlongation(f.storage, source_level, source_level + 1)
    try:
        p.prolongate(f, source_level, flag)
    finally:
        p.close()


def _fmg_arguments(cycles_per_level, post_cycle, post_prolongate):
    """ctypes arguments of hyteg_host_fmg_create: the cycle counts (a number: the scalar form) and the two callbacks.  An exception
    raised in a callback cannot cross the C frames: it is kept in `state` and raised by solve()."""
    if np.ndim(cycles_per_level) == 0:
        counts, n = (_u * 1)(int(cycles_per_level)), 0
    else:
        counts, n = (_u * max(1, len(cycles_per_level)))(*[int(v) for v in cycles_per_level]), len(cycles_per_level)
        if n == 0:
            raise ValueError("fmg: cycles_per_level is empty")  # 0 entries would select the scalar form
    state = {"exception": None}

    def trampoline(fn):
        if fn is None:
            return LEVEL_CB()  # a null function pointer

        def call(level, _user):
            try:
                if state["exception"] is None:
                    fn(int(level))
            except BaseException as e:  # noqa: BLE001 -- re-raised by solve()
                state["exception"] = e

        return LEVEL_CB(call)

    return counts, n, trampoline(post_cycle), trampoline(post_prolongate), state


def _raise_callback_exception(solver):
    state = getattr(solver, "_callbacks", (None, None, None))[2]
    if state and state["exception"] is not None:
        exc, state["exception"] = state["exception"], None
        raise exc


class Solver:
    def __init__(self, handle):
        self.h = handle

    @classmethod
    def gmg(cls, storage, min_level, max_level, smoother=JACOBI, relax=2.0 / 3.0, pre=3, post=3, wcycle=False, cg_max_iter=1000,
            cg_tol=1e-14):
        if smoother == CHEBYSHEV:
            raise ValueError("Solver.gmg: the Chebyshev smoother needs an order and spectral radii, use Solver.gmg_chebyshev")
        h = _vp()
        _ck(lib().hyteg_host_gmg_create(storage.h, min_level, max_level, smoother, float(relax), pre, post, int(wcycle),
                                        cg_max_iter, float(cg_tol), C.byref(h)), "gmg_create")
        return cls(h)

    @classmethod
    def chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3):
        """hyteg::ChebyshevSmoother< P1ConstantLaplaceOperator >; radii: spectral radius of D^-1 A, one for all levels or one per level"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_chebyshev_create(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower), C.byref(h)),
            "chebyshev_create")
        return cls(h)

    @classmethod
    def gmg_chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3, pre=1, post=1, wcycle=False, cg_max_iter=1000,
                      cg_tol=1e-14):
        """GeometricMultigridSolver smoothing with ChebyshevSmoother( order ): pre / post smoother calls per level"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_gmg_create_chebyshev(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower), pre, post,
                                                  int(wcycle), cg_max_iter, float(cg_tol), C.byref(h)), "gmg_create_chebyshev")
        return cls(h)

    def set_fused(self, on: bool) -> None:
        """ChebyshevSmoother::setFused (of a multigrid solver: its smoother's): fused steps (default) or apply + multElementwise + assign"""
        _ck(lib().hyteg_host_chebyshev_set_fused(self.h, int(bool(on))), "chebyshev_set_fused")

    @classmethod
    def cg(cls, storage, min_level, max_level, max_iter=1000, tol=1e-14, preconditioner=None):
        """hyteg::CGSolver< P1ConstantLaplaceOperator >; preconditioner: any Solver (a multigrid solver, Solver.smoother, a Chebyshev
        smoother), None: the loop without one"""
        h = _vp()
        if preconditioner is None:
            _ck(lib().hyteg_host_cg_create(storage.h, min_level, max_level, max_iter, float(tol), C.byref(h)), "cg_create")
            return cls(h)
        _ck(lib().hyteg_host_cg_create_preconditioned(storage.h, min_level, max_level, max_iter, float(tol), preconditioner.h, C.byref(h)),
            "cg_create_preconditioned")
        self = cls(h)
        self._preconditioner = preconditioner  # stays usable as long as this solver is
        return self

    @classmethod
    def smoother(cls, storage, min_level, max_level, smoother, relax=1.0):
        """a smoother on its own (JACOBI, GAUSS_SEIDEL, SOR, JACOBI_FP32, SYMMETRIC_GAUSS_SEIDEL, SYMMETRIC_SOR) or IDENTITY, the
        IdentityPreconditioner: solve = one smoother call; also what Solver.cg takes as preconditioner"""
        h = _vp()
        _ck(lib().hyteg_host_smoother_create(storage.h, min_level, max_level, int(smoother), float(relax), C.byref(h)), "smoother_create")
        return cls(h)

    def set_use_fused_update(self, on: bool) -> None:
        """CGSolver::setUseFusedUpdate of a preconditioned CG solver: x, r and <r,r> in one pass (default) or the three composed calls"""
        _ck(lib().hyteg_host_cg_set_use_fused_update(self.h, int(bool(on))), "cg_set_use_fused_update")

    @classmethod
    def minres(cls, storage, min_level, max_level, max_iter=1000, rel_tol=1e-16, jacobi_iterations=0):
        """hyteg::MinResSolver< P1ConstantLaplaceOperator >, optionally with JacobiPreconditioner( jacobi_iterations )"""
        h = _vp()
        _ck(lib().hyteg_host_solver_create_minres(storage.h, min_level, max_level, int(max_iter), float(rel_tol), jacobi_iterations, C.byref(h)),
            "solver_create_minres")
        return cls(h)

    @classmethod
    def fmg(cls, storage, gmg_solver, min_level, max_level, cycles_per_level=1, prolongation="linear", post_cycle=None, post_prolongate=None):
        """hyteg::FullMultigridSolver around the multigrid solver `gmg_solver`: from min_level up, cycles_per_level (a number, or one
        per level 0..max_level) cycles, post_cycle( level ), the prolongation to the next level ("linear": P1toP1LinearProlongation,
        "quadratic": P1toP1QuadraticProlongationThroughP2Injection), post_prolongate( level )"""
        kind = {"linear": 0, "quadratic": 1}[prolongation]
        counts, n, cb_cycle, cb_prolongate, state = _fmg_arguments(cycles_per_level, post_cycle, post_prolongate)
        h = _vp()
        _ck(lib().hyteg_host_fmg_create(storage.h, gmg_solver.h, min_level, max_level, counts, n, kind, cb_cycle, None, cb_prolongate, None,
                                        C.byref(h)), "fmg_create")
        self = cls(h)
        self._callbacks = (cb_cycle, cb_prolongate, state)  # the C side keeps the function pointers
        return self

    @classmethod
    def mixed_precision_jacobi(cls, storage, min_level, max_level, relax=2.0 / 3.0, fp32_sweeps=2):
        """MixedPrecisionJacobiSmoother on its own (inside a multigrid solver: Solver.gmg(smoother=JACOBI_FP32))"""
        h = _vp()
        _ck(lib().hyteg_host_mixed_precision_jacobi_create(storage.h, min_level, max_level, float(relax), int(fp32_sweeps), C.byref(h)),
            "mixed_precision_jacobi_create")
        return cls(h)

    def solve(self, laplace: P1ConstantOperator, x: P1Function, b: P1Function, level: int):
        _ck(lib().hyteg_host_solver_solve(self.h, laplace.h, x.h, b.h, level), "solve")
        _raise_callback_exception(self)

    def solve_steps(self, laplace: P1ConstantOperator, x: P1Function, b: P1Function, level: int, steps: int):
        """Solver::solveSteps: `steps` calls of solve, which a smoother may fuse (what a multigrid cycle calls for pre / post smoothing)"""
        _ck(lib().hyteg_host_solver_solve_steps(self.h, laplace.h, x.h, b.h, level, int(steps)), "solve_steps")
        _raise_callback_exception(self)

    def set_use_graphs(self, on: bool) -> None:
        """GeometricMultigridSolver::setUseGraphs: record the launches of a cycle once, replay them as graphs (default off)"""
        _ck(lib().hyteg_host_gmg_set_use_graphs(self.h, int(on)), "gmg_set_use_graphs")

    def set_use_device_scalars(self, on: bool, single_launch: bool = False) -> None:
        """CGSolver::setUseDeviceScalars / setUseSingleLaunch (for a multigrid solver: of its coarse-grid CG)"""
        _ck(lib().hyteg_host_cg_set_use_device_scalars(self.h, int(bool(on)) | (2 if single_launch else 0)), "cg_set_use_device_scalars")

    @property
    def iterations(self) -> int:
        n = _i(0)
        _ck(lib().hyteg_host_cg_iterations(self.h, C.byref(n)), "cg_iterations")
        return n.value

    @property
    def replayed_cycles(self) -> int:
        n = _i(0)
        _ck(lib().hyteg_host_gmg_replayed_cycles(self.h, C.byref(n)), "gmg_replayed_cycles")
        return n.value

    def close(self):
        if self.h:
            lib().hyteg_host_solver_destroy(self.h)
            self.h = None


# ---- P2 on a single macro-cell (first version) ----
class P1StokesFunction:
    """hyteg::P1StokesFunction<double>: velocity components u, v, w (boundary types of the storage) and pressure p (all inner)"""

    def __init__(self, storage: Storage, name: str, min_level: int, max_level: int):
        self.storage, self.min_level, self.max_level = storage, min_level, max_level
        h = _vp()
        _ck(lib().hyteg_host_stokes_function_create(storage.h, name.encode(), min_level, max_level, C.byref(h)), "stokes_function_create")
        self.h = h
        self.components = []
        for k in range(4):
            c = _vp()
            _ck(lib().hyteg_host_stokes_function_component(self.h, k, C.byref(c)), "stokes_function_component")
            self.components.append(P1Function(storage, "", min_level, max_level, _borrowed=c))
        self.u, self.v, self.w, self.p = self.components
        self.uvw = self.components[:3]

    def set_velocity_boundary_condition(self, bc: BoundaryCondition, component=None):
        """the condition of the velocity (component: of u, v or w alone); the pressure stays all-inner"""
        for f in self.uvw if component is None else [self.uvw[component]]:
            f.set_boundary_condition(bc)

    def assign(self, scalars, funcs, level, flag=All):
        sc = np.ascontiguousarray(scalars, dtype=np.float64)
        arr = (_vp * len(funcs))(*[f.h for f in funcs])
        _ck(lib().hyteg_host_stokes_function_assign(self.h, len(funcs), sc.ctypes.data_as(_dp), arr, level, flag), "stokes_function_assign")

    def dot(self, other, level, flag=All):
        out = _d()
        _ck(lib().hyteg_host_stokes_function_dot(self.h, other.h, level, flag, C.byref(out)), "stokes_function_dot")
        return out.value

    def close(self):
        if self.h:
            lib().hyteg_host_stokes_function_destroy(self.h)
        self.h = None


def project_mean(pressure: P1Function, level: int):
    """hyteg::vertexdof::projectMean"""
    _ck(lib().hyteg_host_project_mean(pressure.h, level), "project_mean")


class P1P1StokesOperator:
    """hyteg::P1P1StokesOperator: vector Laplace + divT + div + PSPG"""

    def __init__(self, storage: Storage, min_level: int, max_level: int):
        self.storage = storage
        h = _vp()
        _ck(lib().hyteg_host_stokes_operator_create(storage.h, min_level, max_level, C.byref(h)), "stokes_operator_create")
        self.h = h

    def apply(self, src: P1StokesFunction, dst: P1StokesFunction, level, flag):
        _ck(lib().hyteg_host_stokes_operator_apply(self.h, src.h, dst.h, level, flag), "stokes_operator_apply")

    def close(self):
        if self.h:
            lib().hyteg_host_stokes_operator_destroy(self.h)
        self.h = None


class P1ProjectNormalOperator:
    """hyteg::P1ProjectNormalOperator: ( u, v, w ) -= ( ( u, v, w ) . n ) n at the boundary points `flag` selects.  normal(x, y, z) ->
    (nx, ny, nz), not necessarily of unit length, is called once per boundary point and level, here in the constructor; an exception
    it raises ends the constructor and is the cause of the HytegHostError."""
    _prefix = "hyteg_host_project_normal"

    def __init__(self, storage: Storage, min_level: int, max_level: int, normal):
        self.storage = storage

        def call(_user, xyz, out):
            global _hook_exception
            try:
                n = normal(xyz[0], xyz[1], xyz[2])
                out[0], out[1], out[2] = float(n[0]), float(n[1]), float(n[2])
                return 0
            except BaseException as e:  # noqa: BLE001 - must not propagate into the C frames
                if _hook_exception is None:
                    _hook_exception = e
                return 1

        h = _vp()
        _ck(getattr(lib(), self._prefix + "_create")(storage.h, min_level, max_level, NORMAL_CB(call), None, C.byref(h)),
            "project_normal_create")
        self.h = h

    def project(self, target, level, flag=FreeslipBoundary):
        """target: a Stokes function of the operator's discretisation, or its three velocity components"""
        if isinstance(target, (list, tuple)):
            u, v, w = target
            _ck(getattr(lib(), self._prefix + "_project")(self.h, u.h, v.h, w.h, level, flag), "project_normal_project")
        else:
            _ck(getattr(lib(), self._prefix + "_project_stokes")(self.h, target.h, level, flag), "project_normal_project")

    def close(self):
        if self.h:
            getattr(lib(), self._prefix + "_destroy")(self.h)
        self.h = None


class P2ProjectNormalOperator(P1ProjectNormalOperator):
    """hyteg::P2ProjectNormalOperator: the projection on the vertex DoFs and, with normals evaluated at the midpoints of the
    micro-edges, on the edge DoFs of three P2Functions or of a TaylorHoodFunction"""
    _prefix = "hyteg_host_p2_project_normal"


class StrongFreeSlipWrapper:
    """hyteg::StrongFreeSlipWrapper< Operator, ProjectNormalOperator, pre_projection >: op followed by the projection (and preceded
    by it on a copy of the source with pre_projection); flag None (0) switches the projections off"""

    def __init__(self, op, projection, flag=FreeslipBoundary, pre_projection=False):
        self.op, self.projection, self.pre_projection = op, projection, bool(pre_projection)
        self._prefix = "hyteg_host_th_freeslip" if isinstance(op, TaylorHoodStokesOperator) else "hyteg_host_stokes_freeslip"
        h = _vp()
        _ck(getattr(lib(), self._prefix + "_wrapper_create")(op.h, projection.h, int(flag), int(self.pre_projection), C.byref(h)),
            "freeslip_wrapper_create")
        self.h = h

    def apply(self, src, dst, level, flag):
        _ck(getattr(lib(), self._prefix + "_wrapper_apply")(self.h, src.h, dst.h, level, flag), "freeslip_wrapper_apply")

    def close(self):
        if self.h:
            getattr(lib(), self._prefix + "_wrapper_destroy")(self.h)
        self.h = None


class _FreeSlipMinres:
    """MinResSolver< StrongFreeSlipWrapper< ... > >: what StokesSolver.minres / TaylorHoodSolver.minres return with free_slip=True"""

    def __init__(self, prefix, storage, min_level, max_level, max_iter, rel_tol, preconditioner, pre_projection):
        self._prefix = prefix
        h = _vp()
        _ck(getattr(lib(), prefix + "_minres_create")(storage.h, min_level, max_level, int(max_iter), float(rel_tol),
                                                      {"identity": 0, "pressure": 1, "block": 2}[preconditioner], int(bool(pre_projection)),
                                                      C.byref(h)), "freeslip_minres_create")
        self.h = h

    @property
    def minres_iterations(self) -> int:
        n = _i(0)
        _ck(getattr(lib(), self._prefix + "_minres_iterations")(self.h, C.byref(n)), "freeslip_minres_iterations")
        return n.value

    def solve(self, op: StrongFreeSlipWrapper, x, b, level: int):
        if not isinstance(op, StrongFreeSlipWrapper):
            raise TypeError("a solver created with free_slip=True solves a StrongFreeSlipWrapper")
        _ck(getattr(lib(), self._prefix + "_minres_solve")(self.h, op.h, x.h, b.h, level), "freeslip_minres_solve")

    def close(self):
        if self.h:
            getattr(lib(), self._prefix + "_minres_destroy")(self.h)
        self.h = None


class StokesSolver:
    def __init__(self, handle, keep=()):
        self.h = handle
        self._keep = keep

    @classmethod
    def uzawa(cls, storage, min_level, max_level, relax, velocity_iterations=2, velocity_smoother=GAUSS_SEIDEL, velocity_relax=1.0):
        """hyteg::UzawaSmoother< P1P1StokesOperator > over StokesVelocityBlockBlockDiagonalPreconditioner( scalar smoother )"""
        h = _vp()
        _ck(lib().hyteg_host_stokes_uzawa_create(storage.h, min_level, max_level, relax, velocity_iterations, velocity_smoother,
                                                 velocity_relax, C.byref(h)), "stokes_uzawa_create")
        return cls(h)

    @classmethod
    def gmg(cls, storage, smoother, min_level, max_level, pre=3, post=3, increment=0, project_mean_after_restriction=True,
            coarse="lu", coarse_max_iter=1000, coarse_rel_tol=1e-16):
        """hyteg::GeometricMultigridSolver< P1P1StokesOperator >; coarse-grid solver on min_level: "lu" = dense direct solve on
        the host (single rank), "minres" = MinResSolver with the pressure-block preconditioner as apps/stokesSphere composes it
        (any number of ranks)"""
        h = _vp()
        _ck(lib().hyteg_host_stokes_gmg_create_with_coarse(storage.h, smoother.h, min_level, max_level, pre, post, increment,
                                                           int(project_mean_after_restriction), {"lu": 0, "minres": 1}[coarse],
                                                           int(coarse_max_iter), float(coarse_rel_tol), C.byref(h)), "stokes_gmg_create")
        return cls(h, keep=(smoother,))

    @classmethod
    def minres(cls, storage, min_level, max_level, max_iter=1000, rel_tol=1e-16, preconditioner="pressure", velocity_steps=2,
               free_slip=False, pre_projection=False):
        """hyteg::MinResSolver< P1P1StokesOperator >; preconditioner "identity", "pressure" (StokesPressureBlockPreconditioner with the
        lumped inverse mass operator) or "block" (StokesBlockDiagonalPreconditioner: V(2,2) Laplace cycles on the velocity).
        free_slip=True: the solver of a StrongFreeSlipWrapper with that pre_projection ("identity" or "pressure" only)"""
        if free_slip:
            return _FreeSlipMinres("hyteg_host_stokes_freeslip", storage, min_level, max_level, max_iter, rel_tol, preconditioner,
                                   pre_projection)
        h = _vp()
        _ck(lib().hyteg_host_stokes_minres_create(storage.h, min_level, max_level, int(max_iter), float(rel_tol),
                                                  {"identity": 0, "pressure": 1, "block": 2}[preconditioner], velocity_steps, C.byref(h)),
            "stokes_minres_create")
        return cls(h)

    @property
    def minres_iterations(self) -> int:
        n = _i(0)
        _ck(lib().hyteg_host_stokes_minres_iterations(self.h, C.byref(n)), "stokes_minres_iterations")
        return n.value

    def solve(self, op: P1P1StokesOperator, x: P1StokesFunction, b: P1StokesFunction, level: int):
        _ck(lib().hyteg_host_stokes_solver_solve(self.h, op.h, x.h, b.h, level), "stokes_solver_solve")

    def close(self):
        if self.h:
            lib().hyteg_host_stokes_solver_destroy(self.h)
        self.h = None


def _handles3(fs):
    """three component functions (u, v, w) as an array of handles"""
    fs = list(fs)
    if len(fs) != 3:
        raise HytegHostError("a vector function has three components")
    return (_vp * 3)(*[f.h for f in fs])


class P1ElementwiseAffineEpsilonOperator:
    """hyteg::P1ElementwiseAffineEpsilonOperator( storage, minLevel, maxLevel, viscosity ): -div( 2 mu eps(u) ) on a P1 vector
    function, given as its three component functions (for instance P1StokesFunction.uvw).  The reference takes the viscosity as a
    std::function sampled at the points of a degree-2 rule; here mu is a P1Function that holds values on every level
    min_level..max_level (levels 0..8).  The two coincide where mu is linear on every micro-cell, in particular for mu = 1.  Every
    component is masked by its own boundary condition."""

    def __init__(self, storage: Storage, min_level: int, max_level: int, mu: "P1Function"):
        self.storage = storage
        self.min_level, self.max_level = min_level, max_level
        self.mu = mu  # the operator reads mu on every apply: mu outlives it
        h = _vp()
        _ck(lib().hyteg_host_epsilon_create(storage.h, min_level, max_level, mu.h, C.byref(h)), "epsilon_create")
        self.h = h

    def apply(self, src, dst, level, flag, update=Replace):
        _ck(lib().hyteg_host_epsilon_apply(self.h, _handles3(src), _handles3(dst), level, flag, update), "epsilon apply")

    def compute_inverse_diagonal(self):
        _ck(lib().hyteg_host_epsilon_compute_inverse_diagonal(self.h), "epsilon computeInverseDiagonalOperatorValues")

    def inverse_diagonal(self):
        """the inverse diagonals of the three diagonal blocks: three P1Functions (borrowed: they live as long as the operator)"""
        hs = (_vp * 3)()
        _ck(lib().hyteg_host_epsilon_inverse_diagonal(self.h, hs), "epsilon getInverseDiagonalValues")
        return [P1Function(self.storage, "invdiag", self.min_level, self.max_level, _borrowed=_vp(hs[k])) for k in range(3)]

    def smooth_jac(self, dst, rhs, src, relax, level, flag):
        _ck(lib().hyteg_host_epsilon_smooth_jac(self.h, _handles3(dst), _handles3(rhs), _handles3(src), float(relax), level, flag),
            "epsilon smooth_jac")

    def residual(self, x, b, r, level, flag):
        """r = b - A x as a multigrid cycle forms it (three components each): one fused launch on the inner points, or apply + assign
        with set_fused(False)"""
        _ck(lib().hyteg_host_epsilon_residual(self.h, _handles3(x), _handles3(b), _handles3(r), level, flag), "epsilon residual")

    def estimate_radius(self, level: int, iterations: int) -> float:
        """chebyshev::estimateRadius: spectral radius of D^-1 A by power iterations from a fixed start vector (inverse diagonal
        computed)"""
        r = _d()
        _ck(lib().hyteg_host_epsilon_chebyshev_estimate_radius(self.h, int(level), int(iterations), C.byref(r)), "epsilon estimate_radius")
        return r.value

    def set_fused(self, on: bool):
        """smooth_jac, residual and the steps of the Chebyshev smoother: the fused launches on the inner points (default) or the
        composed passes everywhere"""
        _ck(lib().hyteg_host_epsilon_set_fused(self.h, int(bool(on))), "epsilon set_fused")

    def close(self):
        if self.h:
            lib().hyteg_host_epsilon_destroy(self.h)
            self.h = None


class EpsilonSolver:
    """The solvers instantiated for P1ElementwiseAffineEpsilonOperator, acting on three component functions: CGSolver,
    GeometricMultigridSolver (the linear P1 transfer on every component, CG on the coarsest level) with a weighted-Jacobi or a
    Chebyshev smoother, and the smoothers on their own.  Built by the class methods; mirrors DivKGradSolver."""

    def __init__(self, storage, h, keep=None):
        self.storage, self.h, self._keep = storage, h, keep

    @classmethod
    def cg(cls, storage, min_level, max_level, max_iter=1000, tol=1e-14, preconditioner=None):
        """hyteg::CGSolver< P1ElementwiseAffineEpsilonOperator >; preconditioner: an EpsilonSolver or None"""
        h = _vp()
        _ck(lib().hyteg_host_epsilon_cg_create(storage.h, min_level, max_level, max_iter, float(tol),
                                               preconditioner.h if preconditioner is not None else None, C.byref(h)), "epsilon cg_create")
        return cls(storage, h, preconditioner)

    @classmethod
    def gmg(cls, storage, min_level, max_level, smoother=JACOBI, relax=2.0 / 3.0, pre=3, post=3, wcycle=False, cg_max_iter=1000, cg_tol=1e-14):
        """hyteg::GeometricMultigridSolver with WeightedJacobiSmoother( relax ) (the operator has no Gauss-Seidel sweep)"""
        if smoother != JACOBI:
            raise HytegHostError("EpsilonSolver.gmg: smoother JACOBI (gmg_chebyshev for the Chebyshev smoother)")
        h = _vp()
        _ck(lib().hyteg_host_epsilon_gmg_create(storage.h, min_level, max_level, float(relax), pre, post, int(bool(wcycle)), cg_max_iter,
                                                float(cg_tol), C.byref(h)), "epsilon gmg_create")
        return cls(storage, h)

    @classmethod
    def chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3):
        """hyteg::ChebyshevSmoother< P1ElementwiseAffineEpsilonOperator > on its own (solve = one smoother call)"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_epsilon_chebyshev_create(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower), C.byref(h)),
            "epsilon chebyshev_create")
        return cls(storage, h)

    @classmethod
    def gmg_chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3, pre=1, post=1, wcycle=False, cg_max_iter=1000,
                      cg_tol=1e-14):
        """the multigrid solver smoothing with ChebyshevSmoother( order ); radii: one spectral radius
        (P1ElementwiseAffineEpsilonOperator.estimate_radius) or one per level"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_epsilon_gmg_create_chebyshev(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower), pre,
                                                          post, int(bool(wcycle)), cg_max_iter, float(cg_tol), C.byref(h)),
            "epsilon gmg_create_chebyshev")
        return cls(storage, h)

    @classmethod
    def smoother(cls, storage, min_level, max_level, smoother=JACOBI, relax=1.0):
        """WeightedJacobiSmoother( relax ) (JACOBI) or IdentityPreconditioner (IDENTITY) on its own"""
        if smoother not in (JACOBI, IDENTITY):
            raise HytegHostError("EpsilonSolver.smoother: JACOBI or IDENTITY (the epsilon operator has no SOR sweep)")
        h = _vp()
        _ck(lib().hyteg_host_epsilon_smoother_create(storage.h, min_level, max_level, {JACOBI: 0, IDENTITY: -1}[smoother], float(relax),
                                                     C.byref(h)), "epsilon smoother_create")
        return cls(storage, h)

    @property
    def iterations(self) -> int:
        """CGSolver::getIterations of the last solve (EpsilonSolver.cg)"""
        n = _i(0)
        _ck(lib().hyteg_host_epsilon_cg_iterations(self.h, C.byref(n)), "epsilon cg_iterations")
        return n.value

    def solve(self, op: P1ElementwiseAffineEpsilonOperator, xs, bs, level):
        """xs, bs: three component functions each"""
        _ck(lib().hyteg_host_epsilon_solver_solve(self.h, op.h, _handles3(xs), _handles3(bs), level), "epsilon solve")

    def close(self):
        if self.h:
            lib().hyteg_host_epsilon_solver_destroy(self.h)
            self.h = None


class P1P1EpsilonStokesOperator:
    """hyteg::P1P1ElementwiseAffineEpsilonStokesOperator( storage, minLevel, maxLevel, viscosity ): the epsilon operator on the
    velocity, div / divT and the PSPG block; mu: a P1Function as for P1ElementwiseAffineEpsilonOperator"""

    def __init__(self, storage: Storage, min_level: int, max_level: int, mu: "P1Function"):
        self.storage, self.mu = storage, mu
        h = _vp()
        _ck(lib().hyteg_host_epsilon_stokes_create(storage.h, min_level, max_level, mu.h, C.byref(h)), "epsilon_stokes_create")
        self.h = h

    def apply(self, src: "P1StokesFunction", dst: "P1StokesFunction", level, flag):
        _ck(lib().hyteg_host_epsilon_stokes_apply(self.h, src.h, dst.h, level, flag), "epsilon_stokes_apply")

    def close(self):
        if self.h:
            lib().hyteg_host_epsilon_stokes_destroy(self.h)
        self.h = None


class EpsilonStokesSolver:
    """The solver instantiated for P1P1EpsilonStokesOperator: MinResSolver (class method minres)"""

    def __init__(self, handle, keep=()):
        self.h = handle
        self._keep = keep

    @classmethod
    def minres(cls, storage, min_level, max_level, max_iter=1000, rel_tol=1e-16, preconditioner="pressure", mu=None, velocity_cycles=1,
               smoother="chebyshev", order=2, radii=None, relax=2.0 / 3.0, pre=1, post=1, cg_max_iter=1000, cg_tol=1e-14):
        """hyteg::MinResSolver< P1P1ElementwiseAffineEpsilonStokesOperator >; preconditioner "identity", "pressure"
        (StokesPressureBlockPreconditioner with the lumped inverse mass operator, the reference's stokesMinResSolver),
        "pressure_viscosity" (pressure action x.p = mu .* invLumpedMass .* b.p; needs mu, the viscosity function), or the
        block-diagonal ones with a velocity action: "block" (velocity_cycles multigrid V-cycles on the epsilon operator, the lumped
        inverse mass on the pressure) and "block_viscosity" (the same with the pressure action of "pressure_viscosity").  Both need
        mu, the viscosity of the operator.  Their cycle smooths pre = post times with smoother "chebyshev" (of the given order; radii:
        None = estimated per level at construction, one spectral radius, or one per level) or "jacobi" (relax), and solves the coarsest
        level by CG to cg_tol: a symmetric positive definite action, as MINRES needs (any other smoother or pre != post raises)."""
        kinds = {"identity": 0, "pressure": 1, "pressure_viscosity": 2, "block": 3, "block_viscosity": 4}
        if preconditioner not in kinds:
            raise HytegHostError(f"EpsilonStokesSolver.minres: unknown preconditioner {preconditioner!r}")
        kind = kinds[preconditioner]
        if kind in (2, 3, 4) and mu is None:
            raise HytegHostError(f"EpsilonStokesSolver.minres: the {preconditioner} preconditioner needs mu")
        h = _vp()
        if kind >= 3:
            if smoother not in ("chebyshev", "jacobi"):
                raise HytegHostError("EpsilonStokesSolver.minres: smoother 'chebyshev' or 'jacobi' (an SOR sweep is not symmetric)")
            if pre != post:
                raise HytegHostError("EpsilonStokesSolver.minres: a symmetric cycle needs pre == post")
            keep, ptr, n = (None, None, 0) if radii is None else _radii(radii)
            _ck(lib().hyteg_host_epsilon_stokes_minres_create_block(storage.h, min_level, max_level, int(max_iter), float(rel_tol), int(kind == 4),
                                                                    mu.h, int(velocity_cycles), {"jacobi": 0, "chebyshev": 1}[smoother], int(order),
                                                                    ptr, n, float(relax), int(pre), int(post), int(cg_max_iter), float(cg_tol),
                                                                    C.byref(h)), "epsilon_stokes_minres_create_block")
            return cls(h, keep=(mu,))
        _ck(lib().hyteg_host_epsilon_stokes_minres_create(storage.h, min_level, max_level, int(max_iter), float(rel_tol), kind,
                                                          mu.h if kind == 2 else None, C.byref(h)), "epsilon_stokes_minres_create")
        return cls(h, keep=(mu,))

    @property
    def minres_iterations(self) -> int:
        n = _i(0)
        _ck(lib().hyteg_host_epsilon_stokes_minres_iterations(self.h, C.byref(n)), "epsilon_stokes_minres_iterations")
        return n.value

    def solve(self, op: P1P1EpsilonStokesOperator, x: "P1StokesFunction", b: "P1StokesFunction", level: int):
        _ck(lib().hyteg_host_epsilon_stokes_minres_solve(self.h, op.h, x.h, b.h, level), "epsilon_stokes_minres_solve")

    def precondition(self, op: P1P1EpsilonStokesOperator, x: "P1StokesFunction", b: "P1StokesFunction", level: int):
        """the solver's preconditioner on its own: x = M^-1 b"""
        _ck(lib().hyteg_host_epsilon_stokes_minres_precondition(self.h, op.h, x.h, b.h, level), "epsilon_stokes_minres_precondition")

    def close(self):
        if self.h:
            lib().hyteg_host_epsilon_stokes_minres_destroy(self.h)
        self.h = None


class P2Function(_Reductions, _BoundaryConditioned):
    """hyteg::P2Function<double>: vertex DoFs (the P1 cell array) + edge DoFs (EdgeDoFIndexing.hpp layout)"""
    _reduce_fn = "hyteg_host_p2_reduce"
    _bc_prefix = "hyteg_host_p2function"

    def __init__(self, storage: Storage, name: str, min_level: int, max_level: int, _borrowed=None):
        self.storage = storage
        self._borrowed = _borrowed is not None
        if _borrowed is not None:
            self.h = _borrowed
            return
        h = _vp()
        _ck(lib().hyteg_host_p2function_create(storage.h, name.encode(), min_level, max_level, C.byref(h)), "P2Function")
        self.h = h

    def sizes(self, level):
        from . import capi

        return cell_size(level), capi.p2_edge_array_size(level)

    def upload(self, level, vertex, edge, cell=0):
        v = np.ascontiguousarray(vertex, dtype=np.float64)
        e = np.ascontiguousarray(edge, dtype=np.float64)
        assert (v.size, e.size) == self.sizes(level)
        _ck(lib().hyteg_host_p2function_upload(self.h, cell, level, v.ctypes.data, e.ctypes.data), "P2Function.upload")

    def download(self, level, cell=0):
        nv, ne = self.sizes(level)
        v, e = np.empty(nv), np.empty(max(ne, 1))
        _ck(lib().hyteg_host_p2function_download(self.h, cell, level, v.ctypes.data, e.ctypes.data), "P2Function.download")
        return v, e[:ne]

    def interpolate(self, value, level, flag=All, boundary_uid=None):
        if boundary_uid is not None:
            return self._interpolate_on_boundary(value, level, boundary_uid)
        _ck(lib().hyteg_host_p2function_interpolate_constant(self.h, float(value), level, flag), "P2Function.interpolate")

    def _vec(self, fn, scalars, funcs, level, flag):
        n = len(funcs)
        sc = (_d * n)(*[float(v) for v in scalars])
        hs = (_vp * n)(*[f.h for f in funcs])
        _ck(fn(self.h, n, sc, hs, level, flag), "P2Function vector op")

    def assign(self, scalars, funcs, level, flag=All):
        self._vec(lib().hyteg_host_p2function_assign, scalars, funcs, level, flag)

    def add(self, scalars, funcs, level, flag=All):
        self._vec(lib().hyteg_host_p2function_add, scalars, funcs, level, flag)

    def mult_elementwise(self, funcs, level, flag=All):
        hs = (_vp * len(funcs))(*[f.h for f in funcs])
        _ck(lib().hyteg_host_p2function_mult_elementwise(self.h, len(funcs), hs, level, flag), "P2Function.mult_elementwise")

    def dot(self, other, level, flag=All):
        r = _d()
        _ck(lib().hyteg_host_p2function_dot(self.h, other.h, level, flag, C.byref(r)), "P2Function.dot")
        return r.value

    def close(self):
        if self.h and not self._borrowed:
            lib().hyteg_host_p2function_destroy(self.h)
        self.h = None


def p2_prolongate(f: "P2Function", source_level, flag, add=False):
    """hyteg::P2toP2QuadraticProlongation::prolongate / prolongateAndAdd"""
    _ck(lib().hyteg_host_p2_prolongate(f.h, source_level, flag, int(add)), "p2_prolongate")


def p2_restrict(f: "P2Function", source_level, flag):
    """hyteg::P2toP2QuadraticRestriction::restrict"""
    _ck(lib().hyteg_host_p2_restrict(f.h, source_level, flag), "p2_restrict")


class P2ElementwiseLaplaceOperator:
    _create = "hyteg_host_p2operator_create"

    def __init__(self, storage: Storage, min_level: int, max_level: int):
        self.storage = storage
        h = _vp()
        _ck(getattr(lib(), self._create)(storage.h, min_level, max_level, C.byref(h)), type(self).__name__)
        self.h = h

    def element_matrices(self, level, cell=0):
        out = np.empty(600)
        _ck(lib().hyteg_host_p2operator_element_matrices(self.h, cell, level, out.ctypes.data), "element_matrices")
        return out.reshape(6, 10, 10)

    def apply(self, src: P2Function, dst: P2Function, level, flag, update=Replace):
        _ck(lib().hyteg_host_p2operator_apply(self.h, src.h, dst.h, level, flag, update), "P2 apply")

    def compute_inverse_diagonal(self):
        _ck(lib().hyteg_host_p2operator_compute_inverse_diagonal(self.h), "P2 computeInverseDiagonalOperatorValues")

    def inverse_diagonal_into(self, dst: "P2Function", level):
        _ck(lib().hyteg_host_p2operator_inverse_diagonal_copy(self.h, dst.h, level), "P2 inverse diagonal")

    def smooth_jac(self, dst: "P2Function", rhs: "P2Function", src: "P2Function", relax, level, flag=Inner | NeumannBoundary):
        _ck(lib().hyteg_host_p2operator_smooth_jac(self.h, dst.h, rhs.h, src.h, float(relax), level, flag), "P2 smooth_jac")

    def smooth_sor(self, dst: "P2Function", rhs: "P2Function", relax, level, flag=Inner | NeumannBoundary, backwards=False):
        _ck(lib().hyteg_host_p2operator_smooth_sor(self.h, dst.h, rhs.h, float(relax), level, flag, int(bool(backwards))), "P2 smooth_sor")

    def smooth_gs(self, dst: "P2Function", rhs: "P2Function", level, flag=Inner | NeumannBoundary):
        self.smooth_sor(dst, rhs, 1.0, level, flag)

    def cg_solve(self, x: P2Function, b: P2Function, level, max_iter=1000, tol=1e-14):
        it = _i()
        _ck(lib().hyteg_host_p2_cg_solve(self.storage.h, self.h, x.h, b.h, level, max_iter, float(tol), C.byref(it)), "P2 CG")
        return it.value

    def close(self):
        if self.h:
            lib().hyteg_host_p2operator_destroy(self.h)
            self.h = None


class P2Solver:
    """GeometricMultigridSolver< P2ElementwiseLaplaceOperator, P2toP2QuadraticRestriction, P2toP2QuadraticProlongation > with a
    weighted-Jacobi smoother and CG on the coarsest level"""

    def __init__(self, storage: Storage, min_level, max_level, relax=2.0 / 3.0, pre=3, post=3, wcycle=False, cg_max_iter=1000, cg_tol=1e-14,
                 smoother=JACOBI):
        self.storage = storage
        h = _vp()
        kind = {JACOBI: 0, GAUSS_SEIDEL: 1, SOR: 2, SYMMETRIC_GAUSS_SEIDEL: 5, SYMMETRIC_SOR: 6}[smoother]
        _ck(lib().hyteg_host_p2_gmg_create(storage.h, min_level, max_level, kind, float(relax), pre, post, int(bool(wcycle)), cg_max_iter,
                                           float(cg_tol), C.byref(h)), "P2 gmg")
        self.h = h

    @classmethod
    def chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3):
        """hyteg::ChebyshevSmoother< P2ElementwiseLaplaceOperator > on its own (solve = one smoother call)"""
        self = cls.__new__(cls)
        self.storage, self.h = storage, _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_p2_chebyshev_create(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower),
                                                 C.byref(self.h)), "P2 chebyshev")
        return self

    @classmethod
    def gmg_chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3, pre=1, post=1, wcycle=False, cg_max_iter=1000,
                      cg_tol=1e-14):
        """the multigrid solver of this class smoothing with ChebyshevSmoother( order )"""
        self = cls.__new__(cls)
        self.storage, self.h = storage, _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_p2_gmg_create_chebyshev(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower), pre, post,
                                                     int(bool(wcycle)), cg_max_iter, float(cg_tol), C.byref(self.h)), "P2 gmg chebyshev")
        return self

    @classmethod
    def cg(cls, storage, min_level, max_level, max_iter=1000, tol=1e-14, preconditioner=None):
        """hyteg::CGSolver< P2ElementwiseLaplaceOperator >; preconditioner: a P2Solver, None: IdentityPreconditioner"""
        self = cls.__new__(cls)
        self.storage, self.h = storage, _vp()
        self._preconditioner = preconditioner if preconditioner is not None else cls.smoother(storage, min_level, max_level, IDENTITY)
        _ck(lib().hyteg_host_p2_cg_create_preconditioned(storage.h, min_level, max_level, max_iter, float(tol), self._preconditioner.h,
                                                         C.byref(self.h)), "P2 cg_create_preconditioned")
        return self

    @classmethod
    def smoother(cls, storage, min_level, max_level, smoother, relax=1.0):
        """a P2 smoother on its own (JACOBI, GAUSS_SEIDEL, SOR, SYMMETRIC_GAUSS_SEIDEL, SYMMETRIC_SOR) or IDENTITY"""
        self = cls.__new__(cls)
        self.storage, self.h = storage, _vp()
        _ck(lib().hyteg_host_p2_smoother_create(storage.h, min_level, max_level, int(smoother), float(relax), C.byref(self.h)), "P2 smoother_create")
        return self

    @property
    def iterations(self) -> int:
        """CGSolver::getIterations of the last solve (P2Solver.cg)"""
        n = _i(0)
        _ck(lib().hyteg_host_p2_cg_iterations(self.h, C.byref(n)), "P2 cg_iterations")
        return n.value

    @classmethod
    def fmg(cls, storage, gmg_solver, min_level, max_level, cycles_per_level=1, post_cycle=None, post_prolongate=None):
        """hyteg::FullMultigridSolver around the P2 multigrid solver `gmg_solver`, prolongating with P2toP2QuadraticProlongation;
        arguments as for Solver.fmg"""
        self = cls.__new__(cls)
        self.storage, self.h = storage, _vp()
        counts, n, cb_cycle, cb_prolongate, state = _fmg_arguments(cycles_per_level, post_cycle, post_prolongate)
        _ck(lib().hyteg_host_p2_fmg_create(storage.h, gmg_solver.h, min_level, max_level, counts, n, cb_cycle, None, cb_prolongate, None,
                                           C.byref(self.h)), "P2 fmg_create")
        self._callbacks = (cb_cycle, cb_prolongate, state)
        return self

    def solve(self, op, x: "P2Function", b: "P2Function", level):
        _ck(lib().hyteg_host_p2_solver_solve(self.h, op.h, x.h, b.h, level), "P2 solve")
        _raise_callback_exception(self)

    def close(self):
        if self.h:
            lib().hyteg_host_p2_solver_destroy(self.h)
            self.h = None


class P2ElementwiseMassOperator:
    """hyteg::P2ElementwiseMassOperator = P2ElementwiseOperator< forms::P2MassForm >: element matrix |e| times the universal P2 mass
    constants"""

    def __init__(self, storage: Storage, min_level: int, max_level: int):
        self.storage = storage
        h = _vp()
        _ck(lib().hyteg_host_p2massoperator_create(storage.h, min_level, max_level, C.byref(h)), "P2ElementwiseMassOperator")
        self.h = h

    def apply(self, src: P2Function, dst: P2Function, level, flag, update=Replace):
        _ck(lib().hyteg_host_p2massoperator_apply(self.h, src.h, dst.h, level, flag, update), "P2 mass apply")

    def close(self):
        if self.h:
            lib().hyteg_host_p2massoperator_destroy(self.h)
            self.h = None


class P2ElementwiseDivKGrad:
    """hyteg::operatorgeneration::P2ElementwiseDivKGrad( storage, minLevel, maxLevel, k ): -div( k grad u ) on P2 with the P2 coefficient
    function k, which the caller interpolates on every level it uses (the operator at level l reads k at level l).  Every apply goes
    through the C-ABI seam hyteg_hip_p2_elementwise_divkgrad_apply_cell_kinds."""

    def __init__(self, storage: Storage, min_level: int, max_level: int, k: P2Function):
        self.storage, self.k = storage, k  # the coefficient must outlive the operator
        h = _vp()
        _ck(lib().hyteg_host_p2divkgrad_create(storage.h, min_level, max_level, k.h, C.byref(h)), "p2divkgrad_create")
        self.h = h

    def apply(self, src: P2Function, dst: P2Function, level, flag, update=Replace):
        _ck(lib().hyteg_host_p2divkgrad_apply(self.h, src.h, dst.h, level, flag, update), "p2divkgrad apply")

    def gemv(self, alpha, src: P2Function, beta, dst: P2Function, level, flag):
        """dst = alpha A src + beta dst"""
        _ck(lib().hyteg_host_p2divkgrad_gemv(self.h, float(alpha), src.h, float(beta), dst.h, level, flag), "p2divkgrad gemv")

    def compute_inverse_diagonal(self):
        _ck(lib().hyteg_host_p2divkgrad_compute_inverse_diagonal(self.h), "computeInverseDiagonalOperatorValues")

    def inverse_diagonal_into(self, dst: P2Function, level):
        _ck(lib().hyteg_host_p2divkgrad_inverse_diagonal_copy(self.h, dst.h, level), "p2divkgrad inverse diagonal")

    def smooth_jac(self, dst: P2Function, rhs: P2Function, src: P2Function, relax, level, flag=Inner | NeumannBoundary):
        _ck(lib().hyteg_host_p2divkgrad_smooth_jac(self.h, dst.h, rhs.h, src.h, float(relax), level, flag), "p2divkgrad smooth_jac")

    def set_fused(self, on: bool):
        """the fused residual / Jacobi / Chebyshev launches (default), or the composed passes everywhere"""
        _ck(lib().hyteg_host_p2divkgrad_set_fused(self.h, int(bool(on))), "p2divkgrad set_fused")

    def chebyshev_fusable(self, level) -> bool:
        """chebyshevFusable( level ): does ChebyshevSmoother take the fused steps on this level?"""
        n = _i(0)
        _ck(lib().hyteg_host_p2divkgrad_chebyshev_fusable(self.h, int(level), C.byref(n)), "p2divkgrad chebyshev_fusable")
        return bool(n.value)

    def residual(self, x, b, r, level, flag=Inner | NeumannBoundary):
        """r = b - A x as the multigrid cycle writes it"""
        _ck(lib().hyteg_host_p2divkgrad_residual(self.h, x.h, b.h, r.h, level, flag), "p2divkgrad residual")

    def close(self):
        if self.h:
            lib().hyteg_host_p2divkgrad_destroy(self.h)
            self.h = None


class P2DivKGradSolver:
    """The solvers instantiated for P2ElementwiseDivKGrad: CGSolver, GeometricMultigridSolver (quadratic P2 transfer, CG on the coarsest
    level) with a weighted-Jacobi or a Chebyshev smoother, FullMultigridSolver, and the smoothers on their own.  Built by the class
    methods; mirrors DivKGradSolver and P2Solver."""

    def __init__(self, storage, h, keep=None):
        self.storage, self.h, self._keep = storage, h, keep

    @classmethod
    def cg(cls, storage, min_level, max_level, max_iter=1000, tol=1e-14, preconditioner=None):
        """hyteg::CGSolver< P2ElementwiseDivKGrad >; preconditioner: a P2DivKGradSolver or None"""
        h = _vp()
        _ck(lib().hyteg_host_p2divkgrad_cg_create(storage.h, min_level, max_level, max_iter, float(tol),
                                                  preconditioner.h if preconditioner is not None else None, C.byref(h)), "p2divkgrad cg_create")
        return cls(storage, h, preconditioner)

    @classmethod
    def gmg(cls, storage, min_level, max_level, smoother=JACOBI, relax=2.0 / 3.0, pre=3, post=3, wcycle=False, cg_max_iter=1000, cg_tol=1e-14):
        """hyteg::GeometricMultigridSolver with WeightedJacobiSmoother( relax ) (the operator has no Gauss-Seidel sweep)"""
        if smoother != JACOBI:
            raise HytegHostError("P2DivKGradSolver.gmg: smoother JACOBI (gmg_chebyshev for the Chebyshev smoother)")
        h = _vp()
        _ck(lib().hyteg_host_p2divkgrad_gmg_create(storage.h, min_level, max_level, float(relax), pre, post, int(bool(wcycle)), cg_max_iter,
                                                   float(cg_tol), C.byref(h)), "p2divkgrad gmg_create")
        return cls(storage, h)

    @classmethod
    def chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3):
        """hyteg::ChebyshevSmoother< P2ElementwiseDivKGrad > on its own (solve = one smoother call)"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_p2divkgrad_chebyshev_create(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower),
                                                         C.byref(h)), "p2divkgrad chebyshev_create")
        return cls(storage, h)

    @classmethod
    def gmg_chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3, pre=1, post=1, wcycle=False, cg_max_iter=1000,
                      cg_tol=1e-14):
        """the multigrid solver smoothing with ChebyshevSmoother( order ); radii: one spectral radius (estimate_radius) or one per level"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_p2divkgrad_gmg_create_chebyshev(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower), pre,
                                                             post, int(bool(wcycle)), cg_max_iter, float(cg_tol), C.byref(h)),
            "p2divkgrad gmg_create_chebyshev")
        return cls(storage, h)

    @classmethod
    def fmg(cls, storage, gmg_solver, min_level, max_level, cycles_per_level=1):
        """hyteg::FullMultigridSolver around the multigrid solver `gmg_solver`, prolongating with P2toP2QuadraticProlongation;
        cycles_per_level: one count, or one per level"""
        counts = [cycles_per_level] if isinstance(cycles_per_level, int) else list(cycles_per_level)
        arr = (C.c_uint * len(counts))(*counts)
        h = _vp()
        _ck(lib().hyteg_host_p2divkgrad_fmg_create(storage.h, gmg_solver.h, min_level, max_level, arr, 0 if isinstance(cycles_per_level, int) else len(counts),
                                                   C.byref(h)), "p2divkgrad fmg_create")
        return cls(storage, h, gmg_solver)

    @classmethod
    def smoother(cls, storage, min_level, max_level, smoother=JACOBI, relax=1.0):
        """WeightedJacobiSmoother( relax ) (JACOBI) or IdentityPreconditioner (IDENTITY) on its own"""
        h = _vp()
        _ck(lib().hyteg_host_p2divkgrad_smoother_create(storage.h, min_level, max_level, {JACOBI: 0, IDENTITY: -1}[smoother], float(relax),
                                                        C.byref(h)), "p2divkgrad smoother_create")
        return cls(storage, h)

    @property
    def iterations(self) -> int:
        """CGSolver::getIterations of the last solve (P2DivKGradSolver.cg)"""
        n = _i(0)
        _ck(lib().hyteg_host_p2divkgrad_cg_iterations(self.h, C.byref(n)), "p2divkgrad cg_iterations")
        return n.value

    def solve(self, op: P2ElementwiseDivKGrad, x: P2Function, b: P2Function, level):
        _ck(lib().hyteg_host_p2divkgrad_solver_solve(self.h, op.h, x.h, b.h, level), "p2divkgrad solve")

    def close(self):
        if self.h:
            lib().hyteg_host_p2divkgrad_solver_destroy(self.h)
            self.h = None


class P2ConstantLaplaceOperator(P2ElementwiseLaplaceOperator):
    """hyteg::P2ConstantLaplaceOperator: assembles the stencils of its four sub-operators itself (P2Elements3D) and hands them to
    the C-ABI's kernel seam; one kernel pass for all four"""
    _create = "hyteg_host_p2operator_create_constant"

    def inner_stencils(self, level, cell=0):
        """values of the v2v | e2v | v2e | e2e maps of a local cell (order: hyteg_hip_p2_constant_stencil_layout)"""
        out, n = np.empty(512), C.c_int(0)
        _ck(lib().hyteg_host_p2operator_constant_stencils(self.h, cell, level, out.ctypes.data_as(_dp), 512, C.byref(n)), "constant_stencils")
        return out[:n.value].copy()


class TaylorHoodFunction:
    """hyteg::P2P1TaylorHoodFunction<double>: three P2 velocity components and a P1 pressure (all-inner boundary condition)"""

    def __init__(self, storage: Storage, name: str, min_level: int, max_level: int):
        self.storage = storage
        h = _vp()
        _ck(lib().hyteg_host_th_function_create(storage.h, name.encode(), min_level, max_level, C.byref(h)), "TaylorHoodFunction")
        self.h = h
        self.velocity = []
        for k in range(3):
            c = _vp()
            _ck(lib().hyteg_host_th_function_velocity(self.h, k, C.byref(c)), "th velocity")
            self.velocity.append(P2Function(storage, "", min_level, max_level, _borrowed=c))
        c = _vp()
        _ck(lib().hyteg_host_th_function_pressure(self.h, C.byref(c)), "th pressure")
        self.pressure = P1Function(storage, "", min_level, max_level, _borrowed=c)

    def set_velocity_boundary_condition(self, bc: BoundaryCondition, component=None):
        """the condition of the velocity (component: of one component alone); the pressure stays all-inner"""
        for f in self.velocity if component is None else [self.velocity[component]]:
            f.set_boundary_condition(bc)

    def assign(self, scalars, funcs, level, flag=All):
        n = len(funcs)
        sc = (_d * n)(*[float(v) for v in scalars])
        hs = (_vp * n)(*[f.h for f in funcs])
        _ck(lib().hyteg_host_th_function_assign(self.h, n, sc, hs, level, flag), "th assign")

    def interpolate(self, value, level, flag=All):
        _ck(lib().hyteg_host_th_function_interpolate_constant(self.h, float(value), level, flag), "th interpolate")

    def dot(self, other, level, flag=All):
        r = _d()
        _ck(lib().hyteg_host_th_function_dot(self.h, other.h, level, flag, C.byref(r)), "th dot")
        return r.value

    def project_pressure_mean(self, level):
        _ck(lib().hyteg_host_th_project_pressure_mean(self.h, level), "th projectMean")

    def close(self):
        if self.h:
            lib().hyteg_host_th_function_destroy(self.h)
            self.h = None


class TaylorHoodStokesOperator:
    """hyteg::P2P1TaylorHoodStokesOperator"""

    def __init__(self, storage: Storage, min_level: int, max_level: int):
        self.storage = storage
        h = _vp()
        _ck(lib().hyteg_host_th_operator_create(storage.h, min_level, max_level, C.byref(h)), "TaylorHoodStokesOperator")
        self.h = h

    def apply(self, src, dst, level, flag):
        _ck(lib().hyteg_host_th_operator_apply(self.h, src.h, dst.h, level, flag), "th apply")

    def apply_div(self, src, dst, level, flag):
        _ck(lib().hyteg_host_th_operator_apply_block(self.h, 0, src.h, dst.h, level, flag), "th div")

    def apply_divt(self, src, dst, level, flag):
        _ck(lib().hyteg_host_th_operator_apply_block(self.h, 1, src.h, dst.h, level, flag), "th divT")

    def close(self):
        if self.h:
            lib().hyteg_host_th_operator_destroy(self.h)
            self.h = None


class TaylorHoodSolver:
    def __init__(self, h):
        self.h = h

    @classmethod
    def gmg(cls, storage, min_level, max_level, uzawa_relax=0.4, pre=3, post=3, increment=0, coarse_max_iter=200, coarse_rel_tol=1e-12):
        h = _vp()
        _ck(lib().hyteg_host_th_gmg_create(storage.h, min_level, max_level, float(uzawa_relax), pre, post, increment, coarse_max_iter,
                                           float(coarse_rel_tol), C.byref(h)), "th gmg")
        return cls(h)

    @classmethod
    def minres(cls, storage, min_level, max_level, max_iter=100, rel_tol=1e-10, free_slip=False, pre_projection=False):
        """MinResSolver with the pressure-block preconditioner; free_slip=True: the solver of a StrongFreeSlipWrapper with that
        pre_projection"""
        if free_slip:
            return _FreeSlipMinres("hyteg_host_th_freeslip", storage, min_level, max_level, max_iter, rel_tol, "pressure", pre_projection)
        h = _vp()
        _ck(lib().hyteg_host_th_minres_create(storage.h, min_level, max_level, max_iter, float(rel_tol), C.byref(h)), "th minres")
        return cls(h)

    def solve(self, op, x, b, level):
        _ck(lib().hyteg_host_th_solver_solve(self.h, op.h, x.h, b.h, level), "th solve")

    def close(self):
        if self.h:
            lib().hyteg_host_th_solver_destroy(self.h)
            self.h = None


class P2ViscousBlockEpsilonOperator:
    """hyteg::operatorgeneration::P2ViscousBlockEpsilonOperator( storage, minLevel, maxLevel, mu ): -div( 2 mu eps(u) ) on a P2 vector
    function, given as its three component functions (for instance TaylorHoodFunction.velocity), with the P2 viscosity function mu,
    which the caller interpolates on every level it uses (the operator at level l reads mu at level l; levels 0..8).  Every component is
    masked by its own boundary condition.  Every apply goes through the C-ABI seam hyteg_hip_p2_elementwise_epsilon_apply_cell_kinds."""

    def __init__(self, storage: Storage, min_level: int, max_level: int, mu: P2Function):
        self.storage, self.mu = storage, mu  # the viscosity must outlive the operator
        self.min_level, self.max_level = min_level, max_level
        h = _vp()
        _ck(lib().hyteg_host_p2epsilon_create(storage.h, min_level, max_level, mu.h, C.byref(h)), "p2epsilon_create")
        self.h = h

    def apply(self, src, dst, level, flag, update=Replace):
        _ck(lib().hyteg_host_p2epsilon_apply(self.h, _handles3(src), _handles3(dst), level, flag, update), "p2epsilon apply")

    def gemv(self, alpha, src, beta, dst, level, flag):
        """dst = alpha A src + beta dst"""
        _ck(lib().hyteg_host_p2epsilon_gemv(self.h, float(alpha), _handles3(src), float(beta), _handles3(dst), level, flag), "p2epsilon gemv")

    def compute_inverse_diagonal(self):
        _ck(lib().hyteg_host_p2epsilon_compute_inverse_diagonal(self.h), "p2epsilon computeInverseDiagonalOperatorValues")

    def inverse_diagonal(self):
        """the inverse diagonals of the three diagonal blocks: three P2Functions (borrowed: they live as long as the operator)"""
        hs = (_vp * 3)()
        _ck(lib().hyteg_host_p2epsilon_inverse_diagonal(self.h, hs), "p2epsilon getInverseDiagonalValues")
        return [P2Function(self.storage, "invdiag", self.min_level, self.max_level, _borrowed=_vp(hs[k])) for k in range(3)]

    def smooth_jac(self, dst, rhs, src, relax, level, flag=Inner | NeumannBoundary):
        _ck(lib().hyteg_host_p2epsilon_smooth_jac(self.h, _handles3(dst), _handles3(rhs), _handles3(src), float(relax), level, flag),
            "p2epsilon smooth_jac")

    def set_fused(self, on: bool):
        """the fused residual / Jacobi / Chebyshev launches (default), or the composed passes everywhere"""
        _ck(lib().hyteg_host_p2epsilon_set_fused(self.h, int(bool(on))), "p2epsilon set_fused")

    def chebyshev_fusable(self, level) -> bool:
        """chebyshevFusable( level ): does ChebyshevSmoother take the fused steps on this level?"""
        n = _i(0)
        _ck(lib().hyteg_host_p2epsilon_chebyshev_fusable(self.h, int(level), C.byref(n)), "p2epsilon chebyshev_fusable")
        return bool(n.value)

    def residual(self, x, b, r, level, flag=Inner | NeumannBoundary):
        """r = b - A x as the multigrid cycle writes it; x, b, r: three component functions each"""
        _ck(lib().hyteg_host_p2epsilon_residual(self.h, _handles3(x), _handles3(b), _handles3(r), level, flag), "p2epsilon residual")

    def estimate_radius(self, level: int, iterations: int) -> float:
        """chebyshev::estimateRadius: spectral radius of D^-1 A by power iterations from a fixed start vector (inverse diagonal
        computed)"""
        r = _d()
        _ck(lib().hyteg_host_p2epsilon_chebyshev_estimate_radius(self.h, int(level), int(iterations), C.byref(r)), "p2epsilon estimate_radius")
        return r.value

    def close(self):
        if self.h:
            lib().hyteg_host_p2epsilon_destroy(self.h)
            self.h = None


class P2EpsilonSolver:
    """The solvers instantiated for P2ViscousBlockEpsilonOperator, acting on three component functions: CGSolver,
    GeometricMultigridSolver (quadratic P2 transfer on every component, CG on the coarsest level), ChebyshevSmoother and
    WeightedJacobiSmoother / IdentityPreconditioner on their own.  Built by the class methods; mirrors EpsilonSolver."""

    def __init__(self, storage, h, keep=None):
        self.storage, self.h, self._keep = storage, h, keep

    @classmethod
    def cg(cls, storage, min_level, max_level, max_iter=1000, tol=1e-14, preconditioner=None):
        """hyteg::CGSolver< P2ViscousBlockEpsilonOperator >; preconditioner: a P2EpsilonSolver or None"""
        h = _vp()
        _ck(lib().hyteg_host_p2epsilon_cg_create(storage.h, min_level, max_level, max_iter, float(tol),
                                                 preconditioner.h if preconditioner is not None else None, C.byref(h)), "p2epsilon cg_create")
        return cls(storage, h, preconditioner)

    @classmethod
    def chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3):
        """hyteg::ChebyshevSmoother< P2ViscousBlockEpsilonOperator > on its own (solve = one smoother call)"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_p2epsilon_chebyshev_create(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower),
                                                        C.byref(h)), "p2epsilon chebyshev_create")
        return cls(storage, h)

    @classmethod
    def gmg(cls, storage, min_level, max_level, smoother=JACOBI, relax=2.0 / 3.0, pre=3, post=3, wcycle=False, cg_max_iter=1000, cg_tol=1e-14):
        """hyteg::GeometricMultigridSolver with WeightedJacobiSmoother( relax ) (the operator has no Gauss-Seidel sweep)"""
        if smoother != JACOBI:
            raise HytegHostError("P2EpsilonSolver.gmg: smoother JACOBI (gmg_chebyshev for the Chebyshev smoother)")
        h = _vp()
        _ck(lib().hyteg_host_p2epsilon_gmg_create(storage.h, min_level, max_level, float(relax), pre, post, int(bool(wcycle)), cg_max_iter,
                                                  float(cg_tol), C.byref(h)), "p2epsilon gmg_create")
        return cls(storage, h)

    @classmethod
    def gmg_chebyshev(cls, storage, min_level, max_level, order, radii, upper=1.2, lower=0.3, pre=1, post=1, wcycle=False, cg_max_iter=1000,
                      cg_tol=1e-14):
        """the multigrid solver smoothing with ChebyshevSmoother( order ); radii: one spectral radius
        (P2ViscousBlockEpsilonOperator.estimate_radius) or one per level"""
        h = _vp()
        keep, ptr, n = _radii(radii)
        _ck(lib().hyteg_host_p2epsilon_gmg_create_chebyshev(storage.h, min_level, max_level, int(order), ptr, n, float(upper), float(lower), pre,
                                                            post, int(bool(wcycle)), cg_max_iter, float(cg_tol), C.byref(h)),
            "p2epsilon gmg_create_chebyshev")
        return cls(storage, h)

    @classmethod
    def smoother(cls, storage, min_level, max_level, smoother=JACOBI, relax=1.0):
        """WeightedJacobiSmoother( relax ) (JACOBI) or IdentityPreconditioner (IDENTITY) on its own"""
        h = _vp()
        _ck(lib().hyteg_host_p2epsilon_smoother_create(storage.h, min_level, max_level, {JACOBI: 0, IDENTITY: -1}[smoother], float(relax),
                                                       C.byref(h)), "p2epsilon smoother_create")
        return cls(storage, h)

    @property
    def iterations(self) -> int:
        """CGSolver::getIterations of the last solve (P2EpsilonSolver.cg)"""
        n = _i(0)
        _ck(lib().hyteg_host_p2epsilon_cg_iterations(self.h, C.byref(n)), "p2epsilon cg_iterations")
        return n.value

    def solve(self, op: P2ViscousBlockEpsilonOperator, xs, bs, level):
        _ck(lib().hyteg_host_p2epsilon_solver_solve(self.h, op.h, _handles3(xs), _handles3(bs), level), "p2epsilon solve")

    def close(self):
        if self.h:
            lib().hyteg_host_p2epsilon_solver_destroy(self.h)
            self.h = None


class TaylorHoodEpsilonStokesOperator:
    """hyteg::operatorgeneration::P2P1StokesEpsilonOperator( storage, minLevel, maxLevel, mu ): the P2 epsilon operator on the velocity and
    the div / divT blocks of the Taylor-Hood operator (no stabilisation); mu: a P2Function as for P2ViscousBlockEpsilonOperator"""

    def __init__(self, storage: Storage, min_level: int, max_level: int, mu: P2Function):
        self.storage, self.mu = storage, mu
        h = _vp()
        _ck(lib().hyteg_host_th_epsilon_create(storage.h, min_level, max_level, mu.h, C.byref(h)), "th_epsilon_create")
        self.h = h

    def apply(self, src: TaylorHoodFunction, dst: TaylorHoodFunction, level, flag):
        _ck(lib().hyteg_host_th_epsilon_apply(self.h, src.h, dst.h, level, flag), "th_epsilon_apply")

    def close(self):
        if self.h:
            lib().hyteg_host_th_epsilon_destroy(self.h)
        self.h = None


class TaylorHoodEpsilonSolver:
    """The solver instantiated for TaylorHoodEpsilonStokesOperator: MinResSolver (class method minres)"""

    def __init__(self, handle, keep=()):
        self.h = handle
        self._keep = keep

    @classmethod
    def minres(cls, storage, min_level, max_level, max_iter=1000, rel_tol=1e-16, preconditioner="pressure", mu=None, velocity_cycles=1,
               smoother="chebyshev", order=2, radii=None, relax=2.0 / 3.0, pre=1, post=1, velocity_min_level=None, cg_max_iter=1000,
               cg_tol=1e-14):
        """hyteg::MinResSolver< P2P1StokesEpsilonOperator >; preconditioner "identity", "pressure" (StokesPressureBlockPreconditioner with
        the lumped inverse mass operator, the reference's stokesMinResSolver), "pressure_viscosity" (pressure action
        x.p = mu .* invLumpedMass .* b.p with mu at the vertex DoFs; needs mu, the viscosity function), or the block-diagonal ones with a
        velocity action: "block" (velocity_cycles multigrid V-cycles on the P2 epsilon operator over the levels velocity_min_level (default
        min_level) .. max_level, the lumped inverse mass on the pressure) and "block_viscosity" (the same with the pressure action of
        "pressure_viscosity").  Both need mu, the viscosity of the operator.  Their cycle smooths pre = post times with smoother
        "chebyshev" (of the given order; radii: None = estimated per level at construction, one spectral radius, or one per level) or
        "jacobi" (relax), and solves the coarsest level by CG to cg_tol: a symmetric positive definite action, as MINRES needs (any other
        smoother, pre != post or a looser coarse solve raises)."""
        kinds = {"identity": 0, "pressure": 1, "pressure_viscosity": 2, "block": 3, "block_viscosity": 4}
        if preconditioner not in kinds:
            raise HytegHostError(f"TaylorHoodEpsilonSolver.minres: unknown preconditioner {preconditioner!r}")
        kind = kinds[preconditioner]
        if kind in (2, 3, 4) and mu is None:
            raise HytegHostError(f"TaylorHoodEpsilonSolver.minres: the {preconditioner} preconditioner needs mu")
        h = _vp()
        if kind >= 3:
            if smoother not in ("chebyshev", "jacobi"):
                raise HytegHostError("TaylorHoodEpsilonSolver.minres: smoother 'chebyshev' or 'jacobi' (an SOR sweep is not symmetric)")
            if pre != post:
                raise HytegHostError("TaylorHoodEpsilonSolver.minres: a symmetric cycle needs pre == post")
            if cg_tol > 1e-14:
                raise HytegHostError("TaylorHoodEpsilonSolver.minres: the coarse CG of a MINRES preconditioner runs to 1e-14")
            keep, ptr, n = (None, None, 0) if radii is None else _radii(radii)
            vmin = min_level if velocity_min_level is None else int(velocity_min_level)
            _ck(lib().hyteg_host_th_epsilon_minres_create_block(storage.h, min_level, max_level, int(max_iter), float(rel_tol), int(kind == 4), mu.h,
                                                                vmin, int(velocity_cycles), {"jacobi": 0, "chebyshev": 1}[smoother], int(order), ptr,
                                                                n, float(relax), int(pre), int(post), int(cg_max_iter), float(cg_tol), C.byref(h)),
                "th_epsilon_minres_create_block")
            return cls(h, keep=(mu,))
        _ck(lib().hyteg_host_th_epsilon_minres_create(storage.h, min_level, max_level, int(max_iter), float(rel_tol), kind,
                                                      mu.h if kind == 2 else None, C.byref(h)), "th_epsilon_minres_create")
        return cls(h, keep=(mu,))

    @property
    def minres_iterations(self) -> int:
        n = _i(0)
        _ck(lib().hyteg_host_th_epsilon_minres_iterations(self.h, C.byref(n)), "th_epsilon_minres_iterations")
        return n.value

    def solve(self, op: TaylorHoodEpsilonStokesOperator, x: TaylorHoodFunction, b: TaylorHoodFunction, level: int):
        _ck(lib().hyteg_host_th_epsilon_minres_solve(self.h, op.h, x.h, b.h, level), "th_epsilon_minres_solve")

    def precondition(self, op: TaylorHoodEpsilonStokesOperator, x: TaylorHoodFunction, b: TaylorHoodFunction, level: int):
        """the solver's preconditioner on its own: x = M^-1 b"""
        _ck(lib().hyteg_host_th_epsilon_minres_precondition(self.h, op.h, x.h, b.h, level), "th_epsilon_minres_precondition")

    def close(self):
        if self.h:
            lib().hyteg_host_th_epsilon_minres_destroy(self.h)
        self.h = None


def taylor_hood_form_element_matrix(which, k, coords):
    """10 x 10 padded element matrix of a mixed block: which 0 = div (P2 -> P1), 1 = divT (P1 -> P2); component k"""
    co = np.ascontiguousarray(coords, dtype=np.float64).reshape(12)
    out = np.empty(100)
    _ck(lib().hyteg_host_th_form_element_matrix(which, k, co.ctypes.data_as(_dp), out.ctypes.data_as(_dp)), "th_form_element_matrix")
    return out.reshape(10, 10)
