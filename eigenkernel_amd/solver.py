"""Host-side mirror of the reference's solver dispatch, bound to libek_hip.so via ctypes.

Mirrors src/solver_main.f90:22-100 (`eigen_solver(arg, matrix_A, eigenpairs, proc,
matrix_B)`): the `-s <name>` string selects a back-end; the new arms `hip`, `hip_select`,
`general_hip`, `general_hip_select` forward to the C-ABI (include/ek_hip.h) exactly where
the reference forwards `scalapack`, `scalapack_select`, `general_scalapack`,
`general_scalapack_select` to ScaLAPACK (:55-75).

There is NO CPU fallback here: if libek_hip.so is missing or no GPU is visible the call
raises (LibraryMissing / RuntimeError), as the reference `terminate`s when built without a
back-end (solver_elpa_dummy.f90:21).
"""
import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

from . import descriptor as _d

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EK_HIP_LIB") or os.path.join(_HERE, "csrc", "libek_hip.so")   # env: A/B builds

N_STAGES = 8
SOLVERS = ("hip", "hip_select", "general_hip", "general_hip_select")
# reference solver name each arm replaces (solver_main.f90:55,59,64,66)
REPLACES = {"hip": "scalapack", "hip_select": "scalapack_select",
            "general_hip": "general_scalapack", "general_hip_select": "general_scalapack_select"}


class LibraryMissing(RuntimeError):
    pass


_lib = None
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_llp = ctypes.POINTER(ctypes.c_longlong)
# ek_hip_allgatherv_fn (include/ek_hip.h)
ALLGATHERV_FN = ctypes.CFUNCTYPE(ctypes.c_int, _dp, ctypes.c_longlong, _dp, _llp, _llp, ctypes.c_void_p)
_hook_keepalive = None


def load_library(path=None):
    """Loads libek_hip.so and declares every symbol of include/ek_hip.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise LibraryMissing(
            "libek_hip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C eigenkernel_amd/csrc` (there is no CPU fallback)" % p)
    lib = ctypes.CDLL(p)
    c_int, c_dbl, c_ull = ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
    vp = ctypes.c_void_p
    c_ll = ctypes.c_longlong
    sigs = {
        "ek_hip_version": (c_int, []),
        "ek_hip_init": (c_int, [c_int]),
        "ek_hip_finalize": (c_int, []),
        "ek_hip_stage_name": (ctypes.c_char_p, [c_int]),
        "ek_hip_solve": (c_int, [c_int, c_int, c_int, _dp, _ip, _dp, _ip, _dp, _dp, _ip,
                                 c_int, c_int, c_int, c_int, _dp, c_int]),
        "ek_hip_solve_device": (c_int, [c_int, c_int, c_int, vp, c_int, vp, c_int, vp, vp, c_int,
                                        _dp, c_int]),
        "ek_hip_solve_replicated": (c_int, [c_int, c_int, c_int, _dp, c_int, _dp, c_int, _dp, _dp, _ip,
                                            c_int, c_int, c_int, c_int, _dp, c_int]),
        "ek_hip_solve_device_grid": (c_int, [c_int, c_int, c_int, vp, c_int, vp, c_int, vp, vp, c_int,
                                             c_int, c_int, c_int, c_int, c_int, _dp, c_int]),
        "ek_hip_set_allgatherv": (c_int, [ALLGATHERV_FN, vp]),
        "ek_hip_gather_matrix": (c_int, [c_int, c_int, _dp, _ip, c_int, c_int, c_int, c_int, _dp, c_int]),
        "ek_hip_potrf": (c_int, [c_int, _dp, _ip]),
        "ek_hip_sygst": (c_int, [c_int, _dp, _ip, _dp, _ip, _dp]),
        "ek_hip_sytrd": (c_int, [c_int, _dp, _ip, _dp, _dp, _dp]),
        "ek_hip_sytrd_team": (c_int, [c_int, _dp, _ip, _dp, _dp, _dp, c_int, _llp]),
        "ek_hip_sygst_team": (c_int, [c_int, _dp, _ip, _dp, _ip, c_int]),
        "ek_hip_potrf_team": (c_int, [c_int, _dp, _ip, c_int, _llp]),
        "ek_hip_comm_unique_id": (c_int, [vp, c_int]),
        "ek_hip_comm_init": (c_int, [vp, c_int, c_int, c_int]),
        "ek_hip_comm_attach_host": (c_int, [c_int, c_int]),
        "ek_hip_comm_size": (c_int, []),
        "ek_hip_comm_rank": (c_int, []),
        "ek_hip_comm_destroy": (c_int, []),
        "ek_hip_comm_allreduce_device": (c_int, [vp, ctypes.c_longlong]),
        "ek_hip_stedc": (c_int, [c_int, _dp, _dp, _dp, _ip]),
        "ek_hip_ormtr": (c_int, [c_int, c_int, _dp, _ip, _dp, _dp, _ip]),
        "ek_hip_trtrs": (c_int, [c_int, c_int, _dp, _ip, _dp, _ip]),
        "ek_hip_dgemm": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, _dp, c_int, _dp, c_int,
                                 c_dbl, _dp, c_int, c_int]),
        "ek_hip_malloc": (c_int, [ctypes.POINTER(vp), c_ull]),
        "ek_hip_free": (c_int, [vp]),
        "ek_hip_memcpy_h2d": (c_int, [vp, vp, c_ull]),
        "ek_hip_memcpy_d2h": (c_int, [vp, vp, c_ull]),
        "ek_hip_synchronize": (c_int, []),
        "ek_hip_synth_matrix_device": (c_int, [c_int, c_ull, vp, c_int]),
        "ek_hip_residual_device": (c_int, [c_int, c_int, c_int, vp, c_int, vp, c_int, vp, vp, c_int, _dp, _dp, _dp]),
        "ek_hip_orthogonality_device": (c_int, [c_int, c_int, c_int, c_int, vp, c_int, vp, c_int, _dp]),
        "ek_hip_ipratios_device": (c_int, [c_int, c_int, c_int, vp, c_int, vp, c_int, _dp]),
        "ek_hip_check": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _dp, _ip, _dp, _ip, _dp, _dp, _ip, _dp]),
        "ek_hip_profile_symv": (c_int, [c_int]),
        "ek_hip_debug_sytrd": (c_int, [c_int, c_int, c_int, _dp]),
        "ek_hip_debug_sytrd_team": (c_int, [c_int, c_int, c_int, _dp]),
        "ek_hip_debug_set_sytrd_maxcols": (c_int, [c_int]),
        "ek_hip_debug_sytrd_work_bytes": (ctypes.c_ulonglong, [c_int]),
        "ek_hip_debug_sytrd_split": (c_int, [vp, c_int]),
        "ek_hip_debug_gemm_at": (c_int, [c_int, c_int, c_int, c_int, c_int, vp, c_int, vp, c_int, c_dbl, vp, c_int,
                                         c_int, c_int, _dp]),
        "ek_hip_debug_sytrd_at": (c_int, [c_int, c_int, c_int, vp, vp, vp, _dp]),
        # offs / dims: host tables (or None); the last argument: int variant[8]
        "ek_hip_debug_gemm_desc": (c_int, [c_int] * 5 + [c_dbl, c_dbl, vp, c_int, c_ll, vp, c_int, c_ll, vp, c_int, c_ll]
                                   + [c_int] * 5 + [_llp, _ip, _ip]),
        "ek_hip_debug_gemm_plan": (c_int, [c_int] * 5 + [c_dbl, c_dbl, vp, c_int, c_ll, vp, c_int, c_ll, vp, c_int, c_ll]
                                   + [c_int] * 5 + [_llp, _ip, _ip]),
        "ek_hip_debug_gemm_compact_map": (c_int, [c_int, c_int, c_ll, c_int, _ip, _ip, _ip]),
        "ek_hip_debug_reduce_team": (c_int, [c_int, c_int, c_int, _dp]),
        "ek_hip_profile_symv_get": (c_int, [_dp, ctypes.POINTER(ctypes.c_longlong), _dp]),
        "ek_hip_debug_sy2sb": (c_int, [c_int, _dp, c_int, _dp, c_int, _dp, _ip]),
        "ek_hip_debug_sy2sb_stage": (c_int, [c_int, _dp, c_int, _dp, c_int, _dp, c_int, _ip]),
        "ek_hip_debug_set_sy2sb_flow": (c_int, [c_int, c_int]),
        "ek_hip_debug_sb2st": (c_int, [c_int, _dp, c_int, _dp, _dp, _dp, c_int, c_int, _ip]),
        "ek_hip_debug_sb2st_stage": (c_int, [c_int, _dp, c_int, c_int, c_int, _dp, _dp, _dp, c_int, _dp, c_int, _dp, c_int,
                                             c_int, _ip, _ip]),
        "ek_hip_debug_two_stage_timing": (c_int, [c_int, c_int, c_int, _dp, _ip]),
        "ek_hip_debug_set_two_stage": (c_int, [c_int]),
        "ek_hip_profile_kernels": (c_int, [c_int]),
        "ek_hip_profile_kernels_get": (c_int, [_dp, _llp]),
        "ek_hip_debug_last_solve_stats": (c_int, [_dp, c_int]),
        "ek_hip_debug_sy2sb_team": (c_int, [c_int, _dp, c_int, _dp, c_int, _dp, c_int, _ip, _llp]),
        "ek_hip_debug_sy2sb_team_timing": (c_int, [c_int, c_int, c_int, _dp]),
        "ek_hip_debug_sy2sb_team_profile": (c_int, [c_int, c_int, c_int, c_int, _dp, _dp]),
        "ek_hip_debug_fail_next_chase": (c_int, [c_int]),
        "ek_hip_debug_stedc_team": (c_int, [c_int, c_int, c_int]),
        "ek_hip_debug_potrf_team_profile": (c_int, [c_int, c_int]),
        "ek_hip_debug_potrf_team_profile_get": (c_int, [c_int, _dp]),
        "ek_hip_debug_stedc_team_get": (c_int, [_dp]),
        "ek_hip_debug_stedc": (c_int, [c_int, _dp, _dp, c_int, c_int, c_int, c_int, c_int, _dp, _dp, c_int, _ip, c_int,
                                       _ip]),
        "ek_hip_debug_stedc_zcols": (c_int, [c_int, c_int]),
        "ek_hip_debug_ormtr": (c_int, [c_int, c_int, _dp, c_int, _dp, _dp, c_int, c_int, c_int]),
        "ek_hip_debug_last_pipe_stats": (c_int, [_dp, c_int]),
        "ek_hip_debug_workspace_bytes": (ctypes.c_ulonglong, [c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_ulonglong)]),
        "ek_hip_eigenvalues_device": (c_int, [c_int, c_int, c_int, c_int, vp, c_int, vp, c_int, vp, _dp, c_int]),
        "ek_hip_eigenvalues": (c_int, [c_int, c_int, c_int, c_int, _dp, c_int, _dp, c_int, _dp, _dp, c_int]),
        "ek_hip_stebz": (c_int, [c_int, _dp, _dp, c_int, c_int, _dp]),
        "ek_hip_debug_values_workspace_bytes": (ctypes.c_ulonglong, [c_int, c_int]),
        "ek_hip_debug_set_stebz": (c_int, [c_int]),
        "ek_hip_eigenpairs_device": (c_int, [c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, vp, c_int, vp, c_int,
                                             _ip, _ip, vp, vp, c_int, c_int, _dp, c_int]),
        "ek_hip_eigenpairs": (c_int, [c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, _dp, c_int, _dp, c_int,
                                      _ip, _ip, _dp, _dp, c_int, c_int, _dp, c_int]),
        "ek_hip_stebz_range": (c_int, [c_int, _dp, _dp, c_dbl, c_dbl, _ip, _ip, _dp]),
        "ek_hip_debug_window_workspace_bytes": (ctypes.c_ulonglong, [c_int, c_int, c_int, c_int, c_int]),
        "ek_hip_sygvx_device": (c_int, [c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, vp, c_int, vp, c_int,
                                        _ip, _ip, vp, vp, c_int, c_int, _dp, c_int]),
        "ek_hip_sygvx": (c_int, [c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, _dp, c_int, _dp, c_int,
                                 _ip, _ip, _dp, _dp, c_int, c_int, _dp, c_int]),
        "ek_hip_sygst_ibtype": (c_int, [c_int, c_int, _dp, _ip, _dp, _ip, _dp]),
        "ek_hip_trmm": (c_int, [c_int, c_int, _dp, _ip, _dp, _ip]),
        "ek_hip_debug_sygvx_workspace_bytes": (ctypes.c_ulonglong, [c_int, c_int, c_int, c_int, c_int]),
        "ek_hip_eigenpairs_batched_device": (c_int, [c_int, c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp,
                                                     vp, c_int, c_ll, _ip, _dp]),
        "ek_hip_eigenpairs_batched": (c_int, [c_int, c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp,
                                              _dp, c_int, c_ll, _ip, _dp]),
        # the pointer arrays (double *const *) are passed as ctypes arrays of c_void_p
        "ek_hip_eigenpairs_vbatched_device": (c_int, [c_int, c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip,
                                                      _dp]),
        "ek_hip_eigenpairs_vbatched": (c_int, [c_int, c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp]),
        "ek_hip_sygv_batched_device": (c_int, [c_int, c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp, vp,
                                               c_int, c_ll, _ip, _dp]),
        "ek_hip_sygv_batched": (c_int, [c_int, c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp, _dp, c_int,
                                        c_ll, _ip, _dp]),
        "ek_hip_sygv_vbatched_device": (c_int, [c_int, c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp]),
        "ek_hip_sygv_vbatched": (c_int, [c_int, c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp]),
        "ek_hip_check_batched_device": (c_int, [c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp, vp, c_int, c_ll,
                                                _ip, _dp, _dp, _dp]),
        "ek_hip_check_batched": (c_int, [c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp, _dp, c_int, c_ll,
                                         _ip, _dp, _dp, _dp]),
        "ek_hip_check_vbatched_device": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp, vp, _dp]),
        "ek_hip_check_vbatched": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp, vp, _dp]),
        "ek_hip_check_sygv_batched_device": (c_int, [c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp, vp, c_int,
                                                     c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_check_sygv_batched": (c_int, [c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp, _dp, c_int,
                                              c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_check_sygv_vbatched_device": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp, vp,
                                                      _dp]),
        "ek_hip_check_sygv_vbatched": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp, vp, _dp]),
        "ek_hip_check_sygvx_device": (c_int, [c_int, c_int, c_int, vp, c_int, vp, c_int, vp, vp, c_int, _dp, _dp]),
        "ek_hip_check_sygvx": (c_int, [c_int, c_int, c_int, _dp, c_int, _dp, c_int, _dp, _dp, c_int, _dp, _dp]),
        "ek_hip_eigenpairs_xbatched_device": (c_int, [c_int, c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp,
                                                      vp, c_int, c_ll, _ip, _dp]),
        "ek_hip_eigenpairs_xbatched": (c_int, [c_int, c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp,
                                               _dp, c_int, c_ll, _ip, _dp]),
        "ek_hip_sygv_xbatched_device": (c_int, [c_int, c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp, vp,
                                                c_int, c_ll, _ip, _dp]),
        "ek_hip_sygv_xbatched": (c_int, [c_int, c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp, _dp, c_int,
                                         c_ll, _ip, _dp]),
        "ek_hip_debug_xbatched_chunk": (c_int, [c_int]),
        "ek_hip_eigenpairs_ybatched_device": (c_int, [c_int, c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp,
                                                      vp, c_int, c_ll, _ip, _dp]),
        "ek_hip_eigenpairs_ybatched": (c_int, [c_int, c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp,
                                               _dp, c_int, c_ll, _ip, _dp]),
        "ek_hip_sygv_ybatched_device": (c_int, [c_int, c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp, vp,
                                                c_int, c_ll, _ip, _dp]),
        "ek_hip_sygv_ybatched": (c_int, [c_int, c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp, _dp, c_int,
                                         c_ll, _ip, _dp]),
        "ek_hip_debug_ybatched_chunk": (c_int, [c_int]),
        "ek_hip_eigenpairs_window_batched_device": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int,
                                                            vp, c_int, c_ll, vp, c_int, c_ll, _ip, vp, vp, c_int, c_int,
                                                            c_ll, _ip, _dp]),
        "ek_hip_eigenpairs_window_batched": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, _dp,
                                                     c_int, c_ll, _dp, c_int, c_ll, _ip, _dp, _dp, c_int, c_int, c_ll,
                                                     _ip, _dp]),
        "ek_hip_debug_window_batched_chunk": (c_int, [c_int]),
        "ek_hip_eigenpairs_window_xbatched_device": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int,
                                                             vp, c_int, c_ll, vp, c_int, c_ll, _ip, vp, vp, c_int, c_int,
                                                             c_ll, _ip, _dp]),
        "ek_hip_eigenpairs_window_xbatched": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, _dp,
                                                      c_int, c_ll, _dp, c_int, c_ll, _ip, _dp, _dp, c_int, c_int, c_ll,
                                                      _ip, _dp]),
        "ek_hip_debug_window_xbatched_chunk": (c_int, [c_int]),
        "ek_hip_sygv_window_batched_device": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, vp,
                                                      c_int, c_ll, vp, c_int, c_ll, _ip, vp, vp, c_int, c_int, c_ll,
                                                      _ip, _dp]),
        "ek_hip_sygv_window_batched": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, _dp, c_int,
                                               c_ll, _dp, c_int, c_ll, _ip, _dp, _dp, c_int, c_int, c_ll, _ip, _dp]),
        "ek_hip_sygv_window_xbatched_device": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, vp,
                                                       c_int, c_ll, vp, c_int, c_ll, _ip, vp, vp, c_int, c_int, c_ll,
                                                       _ip, _dp]),
        "ek_hip_sygv_window_xbatched": (c_int, [c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int, c_int, _dp, c_int,
                                                c_ll, _dp, c_int, c_ll, _ip, _dp, _dp, c_int, c_int, c_ll, _ip, _dp]),
        "ek_hip_check_xbatched_device": (c_int, [c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp, vp, c_int,
                                                 c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_check_xbatched": (c_int, [c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp, _dp, c_int, c_ll,
                                          _ip, _dp, _dp, _dp]),
        "ek_hip_debug_check_xbatched_chunk": (c_int, [c_int]),
        "ek_hip_check_window_xbatched_device": (c_int, [c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, _ip, vp, vp,
                                                        c_int, c_int, c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_check_window_xbatched": (c_int, [c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _ip, _dp, _dp,
                                                 c_int, c_int, c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_check_sygv_window_xbatched_device": (c_int, [c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, _ip, vp,
                                                             vp, c_int, c_int, c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_check_sygv_window_xbatched": (c_int, [c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _ip, _dp,
                                                      _dp, c_int, c_int, c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_check_sygv_xbatched_device": (c_int, [c_int, c_int, c_int, vp, c_int, c_ll, vp, c_int, c_ll, vp, vp, c_int,
                                                      c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_check_sygv_xbatched": (c_int, [c_int, c_int, c_int, _dp, c_int, c_ll, _dp, c_int, c_ll, _dp, _dp, c_int,
                                               c_ll, _ip, _dp, _dp, _dp]),
        "ek_hip_debug_vbatched_streams": (c_int, [c_int]),
        "ek_hip_debug_vbatched_last": (c_int, [_dp, _ip]),
        "ek_hip_eigenpairs_xvbatched_device": (c_int, [c_int, c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip,
                                                       _dp]),
        "ek_hip_eigenpairs_xvbatched": (c_int, [c_int, c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp]),
        "ek_hip_sygv_xvbatched_device": (c_int, [c_int, c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp]),
        "ek_hip_sygv_xvbatched": (c_int, [c_int, c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp]),
        "ek_hip_debug_xvbatched_last": (c_int, [_dp, _ip]),
        "ek_hip_eigenpairs_window_xvbatched_device": (c_int, [c_int, c_int, c_int, c_int, _ip, _dp, _dp, _ip, _ip, vp, _ip,
                                                              vp, _ip, _ip, vp, vp, _ip, _ip, _ip, _dp]),
        "ek_hip_eigenpairs_window_xvbatched": (c_int, [c_int, c_int, c_int, c_int, _ip, _dp, _dp, _ip, _ip, vp, _ip, vp,
                                                       _ip, _ip, vp, vp, _ip, _ip, _ip, _dp]),
        "ek_hip_sygv_window_xvbatched_device": (c_int, [c_int, c_int, c_int, c_int, _ip, _dp, _dp, _ip, _ip, vp, _ip, vp,
                                                        _ip, _ip, vp, vp, _ip, _ip, _ip, _dp]),
        "ek_hip_sygv_window_xvbatched": (c_int, [c_int, c_int, c_int, c_int, _ip, _dp, _dp, _ip, _ip, vp, _ip, vp, _ip,
                                                 _ip, vp, vp, _ip, _ip, _ip, _dp]),
        "ek_hip_debug_window_xvbatched_budget": (ctypes.c_longlong, [ctypes.c_longlong]),
        "ek_hip_check_xvbatched_device": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp, vp, _dp]),
        "ek_hip_check_xvbatched": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp, vp, _dp]),
        "ek_hip_check_sygv_xvbatched_device": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp, vp,
                                                       _dp]),
        "ek_hip_check_sygv_xvbatched": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, vp, vp, _ip, _ip, _dp, vp, _dp]),
        "ek_hip_debug_check_xvbatched_last": (c_int, [_dp, _ip]),
        "ek_hip_check_window_xvbatched_device": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, _ip, vp, vp, _ip, _ip,
                                                          _ip, _dp, vp, _dp]),
        "ek_hip_check_window_xvbatched": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, _ip, vp, vp, _ip, _ip,
                                                   _ip, _dp, vp, _dp]),
        "ek_hip_check_sygv_window_xvbatched_device": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, _ip, vp, vp, _ip, _ip,
                                                               _ip, _dp, vp, _dp]),
        "ek_hip_check_sygv_window_xvbatched": (c_int, [c_int, c_int, _ip, vp, _ip, vp, _ip, _ip, vp, vp, _ip, _ip,
                                                        _ip, _dp, vp, _dp]),
        "ek_hip_debug_stage_leaves256": (c_int, [c_int]),
        "ek_hip_debug_set_sygst_direct": (c_int, [c_int]),
        "ek_hip_debug_sygst_scratch": (c_ull, [c_int, ctypes.POINTER(c_ull)]),
        # a triplet list is (nnz, suffix, value)
        "ek_hip_solve_sparse": (c_int, [c_int, c_int, c_int, c_ll, _ip, _dp, c_ll, _ip, _dp, _dp, _dp, _ip,
                                        c_int, c_int, c_int, c_int, _dp, c_int]),
        "ek_hip_check_sparse_device": (c_int, [c_int, c_int, c_ll, _ip, _dp, c_ll, _ip, _dp, vp, vp, c_int,
                                               c_int, c_int, c_int, c_int, _dp, _dp]),
        "ek_hip_check_sparse": (c_int, [c_int, c_int, c_ll, _ip, _dp, c_ll, _ip, _dp, _dp, _dp, c_int,
                                        c_int, c_int, c_int, c_int, _dp, _dp]),
        "ek_hip_sparse_to_dense": (c_int, [c_int, c_ll, _ip, _dp, _dp, c_int]),
        "ek_hip_debug_sparse_check_workspace_bytes": (c_ull, [c_int, c_int, c_ll, c_ll, c_int, c_int, c_int, c_int]),
        "ek_hip_debug_sparse_csr": (c_ll, [c_int, c_ll, _ip, _dp, _llp, _ip, _dp]),
    }
    for name, (res, args) in sigs.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if os.environ.get("EK_HIP_BRINGUP") == "1":   # partial library during development
                continue
            raise   # header / library mismatch
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


EXPORTED_SYMBOLS = (
    "ek_hip_version", "ek_hip_init", "ek_hip_finalize", "ek_hip_stage_name", "ek_hip_solve",
    "ek_hip_solve_device", "ek_hip_solve_replicated", "ek_hip_solve_device_grid",
    "ek_hip_set_allgatherv", "ek_hip_gather_matrix", "ek_hip_potrf", "ek_hip_sygst", "ek_hip_sytrd", "ek_hip_stedc",
    "ek_hip_ormtr", "ek_hip_trtrs", "ek_hip_dgemm", "ek_hip_malloc", "ek_hip_free",
    "ek_hip_memcpy_h2d", "ek_hip_memcpy_d2h", "ek_hip_synchronize", "ek_hip_synth_matrix_device",
    "ek_hip_profile_symv", "ek_hip_profile_symv_get", "ek_hip_debug_sytrd",
    "ek_hip_residual_device", "ek_hip_orthogonality_device", "ek_hip_ipratios_device", "ek_hip_check",
    "ek_hip_sytrd_team", "ek_hip_comm_unique_id", "ek_hip_comm_init", "ek_hip_comm_size", "ek_hip_comm_rank",
    "ek_hip_comm_destroy", "ek_hip_comm_allreduce_device", "ek_hip_debug_sytrd_team", "ek_hip_sygst_team",
    "ek_hip_potrf_team", "ek_hip_debug_reduce_team", "ek_hip_comm_attach_host",
    "ek_hip_debug_set_sytrd_maxcols", "ek_hip_debug_sytrd_work_bytes", "ek_hip_debug_sytrd_at", "ek_hip_debug_sytrd_split", "ek_hip_debug_gemm_at",
    "ek_hip_debug_gemm_desc", "ek_hip_debug_gemm_plan", "ek_hip_debug_gemm_compact_map",
    "ek_hip_debug_sy2sb", "ek_hip_debug_sy2sb_stage", "ek_hip_debug_set_sy2sb_flow", "ek_hip_debug_sb2st", "ek_hip_debug_sb2st_stage", "ek_hip_debug_two_stage_timing", "ek_hip_debug_set_two_stage",
    "ek_hip_profile_kernels", "ek_hip_profile_kernels_get", "ek_hip_debug_last_solve_stats",
    "ek_hip_debug_sy2sb_team", "ek_hip_debug_sy2sb_team_timing", "ek_hip_debug_sy2sb_team_profile", "ek_hip_debug_workspace_bytes", "ek_hip_debug_fail_next_chase", "ek_hip_debug_last_pipe_stats",
    "ek_hip_debug_stedc_team", "ek_hip_debug_stedc_team_get", "ek_hip_debug_stedc",
    "ek_hip_debug_stedc_zcols", "ek_hip_debug_ormtr",
    "ek_hip_debug_potrf_team_profile", "ek_hip_debug_potrf_team_profile_get",
    "ek_hip_eigenvalues_device", "ek_hip_eigenvalues", "ek_hip_stebz",
    "ek_hip_debug_values_workspace_bytes", "ek_hip_debug_set_stebz",
    "ek_hip_eigenpairs_device", "ek_hip_eigenpairs", "ek_hip_stebz_range", "ek_hip_debug_window_workspace_bytes",
    "ek_hip_sygvx_device", "ek_hip_sygvx", "ek_hip_sygst_ibtype", "ek_hip_trmm", "ek_hip_debug_sygvx_workspace_bytes",
    "ek_hip_eigenpairs_batched_device", "ek_hip_eigenpairs_batched",
    "ek_hip_eigenpairs_vbatched_device", "ek_hip_eigenpairs_vbatched",
    "ek_hip_debug_vbatched_streams", "ek_hip_debug_vbatched_last",
    "ek_hip_check_batched_device", "ek_hip_check_batched", "ek_hip_check_vbatched_device", "ek_hip_check_vbatched",
    "ek_hip_sygv_batched_device", "ek_hip_sygv_batched", "ek_hip_sygv_vbatched_device", "ek_hip_sygv_vbatched",
    "ek_hip_check_sygv_batched_device", "ek_hip_check_sygv_batched", "ek_hip_check_sygv_vbatched_device",
    "ek_hip_check_sygv_vbatched", "ek_hip_check_sygvx_device", "ek_hip_check_sygvx",
    "ek_hip_eigenpairs_xbatched_device", "ek_hip_eigenpairs_xbatched", "ek_hip_debug_xbatched_chunk",
    "ek_hip_check_xbatched_device", "ek_hip_check_xbatched", "ek_hip_debug_check_xbatched_chunk",
    "ek_hip_sygv_xbatched_device", "ek_hip_sygv_xbatched",
    "ek_hip_check_sygv_xbatched_device", "ek_hip_check_sygv_xbatched",
    "ek_hip_eigenpairs_xvbatched_device", "ek_hip_eigenpairs_xvbatched", "ek_hip_sygv_xvbatched_device",
    "ek_hip_sygv_xvbatched", "ek_hip_debug_xvbatched_last",
    "ek_hip_eigenpairs_window_xvbatched_device", "ek_hip_eigenpairs_window_xvbatched",
    "ek_hip_sygv_window_xvbatched_device", "ek_hip_sygv_window_xvbatched", "ek_hip_debug_window_xvbatched_budget",
    "ek_hip_check_xvbatched_device", "ek_hip_check_xvbatched", "ek_hip_check_sygv_xvbatched_device",
    "ek_hip_check_sygv_xvbatched", "ek_hip_debug_check_xvbatched_last",
    "ek_hip_debug_stage_leaves256", "ek_hip_debug_set_sygst_direct", "ek_hip_debug_sygst_scratch",
    "ek_hip_solve_sparse", "ek_hip_check_sparse_device", "ek_hip_check_sparse", "ek_hip_sparse_to_dense",
    "ek_hip_debug_sparse_check_workspace_bytes", "ek_hip_debug_sparse_csr",
    "ek_hip_eigenpairs_window_batched_device", "ek_hip_eigenpairs_window_batched", "ek_hip_debug_window_batched_chunk",
    "ek_hip_eigenpairs_window_xbatched_device", "ek_hip_eigenpairs_window_xbatched",
    "ek_hip_debug_window_xbatched_chunk",
    "ek_hip_sygv_window_batched_device", "ek_hip_sygv_window_batched",
    "ek_hip_sygv_window_xbatched_device", "ek_hip_sygv_window_xbatched",
    "ek_hip_check_window_xbatched_device", "ek_hip_check_window_xbatched",
    "ek_hip_check_sygv_window_xbatched_device", "ek_hip_check_sygv_window_xbatched",
    "ek_hip_check_window_xvbatched_device", "ek_hip_check_window_xvbatched",
    "ek_hip_check_sygv_window_xvbatched_device", "ek_hip_check_sygv_window_xvbatched",
    "ek_hip_eigenpairs_ybatched_device", "ek_hip_eigenpairs_ybatched", "ek_hip_sygv_ybatched_device",
    "ek_hip_sygv_ybatched", "ek_hip_debug_ybatched_chunk",
)


def _check(what, A, B, w, Z, n_cols, index1=1, index2=1):
    lib = load_library()
    Z = _farr(Z)
    n = Z.shape[0]
    A_ = _farr(A) if A is not None else None
    B_ = _farr(B) if B is not None else None
    out = np.zeros(max(3, n))
    wv = np.ascontiguousarray(np.asarray(w, dtype=np.float64)) if w is not None else np.zeros(max(n, 1))
    info = lib.ek_hip_check(what, 1 if B is not None else 0, n, n_cols, index1, index2,
                            _P(A_) if A_ is not None else None, _I(_desc_for(A_)) if A_ is not None else None,
                            _P(B_) if B_ is not None else None, _I(_desc_for(B_)) if B_ is not None else None,
                            _P(wv), _P(Z), _I(_desc_for(Z)), _P(out))
    if info:
        raise RuntimeError("ek_hip_check(%d) info=%d" % (what, info))
    return out


def eval_residual_norm(A, values, V, B=None, n_check=None):
    """verifier.f90:207 on the GPU. Returns (A_norm, res_norm_ave, res_norm_max)."""
    n_check = V.shape[1] if n_check is None else n_check
    Zf = np.zeros((V.shape[0], V.shape[0]), order="F"); Zf[:, :V.shape[1]] = V
    wv = np.zeros(V.shape[0]); wv[:len(values)] = values
    out = _check(0, A, B, wv, Zf, n_check)
    return out[0], out[1], out[2]


def eval_orthogonality(V, B=None, index1=1, index2=None):
    """verifier.f90:333 on the GPU."""
    index2 = V.shape[1] if index2 is None else index2
    Zf = np.zeros((V.shape[0], V.shape[0]), order="F"); Zf[:, :V.shape[1]] = V
    return _check(1, None, B, None, Zf, 0, index1, index2)[0]


def get_ipratios(V, S=None, n_vec=None):
    """distribute_matrix.f90:18 on the GPU."""
    n_vec = V.shape[1] if n_vec is None else n_vec
    Zf = np.zeros((V.shape[0], V.shape[0]), order="F"); Zf[:, :V.shape[1]] = V
    return _check(2, None, S, None, Zf, n_vec)[:n_vec].copy()



def _P(a):
    return a.ctypes.data_as(_dp)


def _I(a):
    return a.ctypes.data_as(_ip)


def _farr(a):
    a = np.asarray(a, dtype=np.float64)
    return a if a.flags.f_contiguous else np.asfortranarray(a)


def _desc_for(a, nb=None):
    m, n = a.shape
    nb = min(_d.g_block_size if nb is None else nb, max(min(m, n), 1))
    return _d.descinit(m, n, nb, nb, 0, 0, 0, max(1, a.strides[1] // 8 if n > 1 else m))


# ----------------------------------------------------------------------------- exchange hook
def set_allgatherv(fn):
    """Registers the host exchange hook ek_hip_solve needs on grids larger than 1x1.

    fn(send: ndarray[count], counts: list[int], displs: list[int]) -> ndarray[sum(counts)]
    with MPI_Allgatherv semantics over the grid's ranks in row-major order; None removes it.
    """
    global _hook_keepalive
    lib = load_library()
    if fn is None:
        lib.ek_hip_set_allgatherv(ctypes.cast(None, ALLGATHERV_FN), None)
        _hook_keepalive = None
        return

    n_ranks = getattr(fn, "n_ranks", None)
    if n_ranks is None:
        raise ValueError("the hook must carry .n_ranks (number of ranks of the grid)")

    def thunk(send, count, recv, counts, displs, _user):
        try:
            cs = [int(counts[r]) for r in range(n_ranks)]
            ds = [int(displs[r]) for r in range(n_ranks)]
            count = int(count)
            sv = np.ctypeslib.as_array(send, shape=(max(count, 1),))[:count]
            out = np.asarray(fn(sv, cs, ds), dtype=np.float64)
            total = ds[-1] + cs[-1]
            if out.shape != (total,):
                return 2
            np.ctypeslib.as_array(recv, shape=(max(total, 1),))[:total] = out
            return 0
        except Exception:                     # never let an exception cross the C boundary
            import traceback
            traceback.print_exc()
            return 1

    cb = ALLGATHERV_FN(thunk)
    _hook_keepalive = (cb, thunk, fn)
    lib.ek_hip_set_allgatherv(cb, None)


def torch_allgatherv(dist, group=None):
    """Exchange hook on torch.distributed host tensors (gloo in the CPU tests; with the nccl
    backend pass a gloo side group): pads every piece to the largest and all-gathers."""
    import torch
    world = dist.get_world_size(group)

    def fn(send, counts, displs):
        mx = max(max(counts), 1)
        mine = torch.zeros(mx, dtype=torch.float64)
        mine[:send.shape[0]] = torch.from_numpy(np.ascontiguousarray(send))
        parts = [torch.empty(mx, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        out = np.empty(displs[-1] + counts[-1])
        for r in range(world):
            out[displs[r]:displs[r] + counts[r]] = parts[r][:counts[r]].numpy()
        return out

    fn.n_ranks = world
    return fn


def gather_matrix(M_loc, desc, proc):
    """ek_hip_gather_matrix: the full matrix from every rank's block-cyclic piece (host only)."""
    lib = load_library()
    m, n = int(desc[_d.ROWS_]), int(desc[_d.COLS_])
    full = np.zeros((m, n), order="F")
    info = lib.ek_hip_gather_matrix(m, n, _P(M_loc), _I(desc), proc.n_procs_row, proc.n_procs_col,
                                    proc.my_proc_row, proc.my_proc_col, _P(full), max(1, m))
    if info != 0:
        raise SolverError("ek_hip_gather_matrix failed", info)
    return full


# ----------------------------------------------------------------------------- types
@dataclass
class Process:
    """ek_process_t (processes.f90:6-9)."""
    my_rank: int = 0
    n_procs: int = 1
    context: int = 0
    n_procs_row: int = 1
    n_procs_col: int = 1
    my_proc_row: int = 0
    my_proc_col: int = 0


@dataclass
class EigenpairsBlacs:
    """ek_eigenpairs_blacs_t (eigenpairs_types.f90:7-11); type_number = 2."""
    values: np.ndarray = None
    desc: np.ndarray = None
    Vectors: np.ndarray = None
    type_number: int = 2
    stage_seconds: dict = field(default_factory=dict)
    info: int = 0


class SolverError(RuntimeError):
    """Raised where the reference calls terminate(msg, info) (processes.f90:122-139)."""

    def __init__(self, msg, info):
        super().__init__("%s (info=%d)" % (msg, info))
        self.info = info


# ----------------------------------------------------------------------------- stage-level wrappers
def potrf(B):
    """PDPOTRF('L') (generalized_to_standard.f90:24). Returns (B_with_L_in_lower, info)."""
    lib = load_library()
    B = np.array(_farr(B), order="F", copy=True)
    desc = _desc_for(B)
    info = lib.ek_hip_potrf(B.shape[0], _P(B), _I(desc))
    return B, info


def sygst(A, L):
    """PDSYGST(1,'L') (generalized_to_standard.f90:37)."""
    lib = load_library()
    A = np.array(_farr(A), order="F", copy=True)
    L = _farr(L)
    scale = ctypes.c_double(0.0)
    info = lib.ek_hip_sygst(A.shape[0], _P(A), _I(_desc_for(A)), _P(L), _I(_desc_for(L)),
                            ctypes.byref(scale))
    return A, info


def sytrd(A):
    """PDSYTRD('L') (solver_scalapack_all.f90:59). Returns (A_reflectors, d, e, tau, info)."""
    lib = load_library()
    A = np.array(_farr(A), order="F", copy=True)
    n = A.shape[0]
    d = np.zeros(max(n, 1)); e = np.zeros(max(n, 1)); tau = np.zeros(max(n, 1))
    info = lib.ek_hip_sytrd(n, _P(A), _I(_desc_for(A)), _P(d), _P(e), _P(tau))
    return A, d[:n], e[:max(n - 1, 0)], tau[:max(n - 1, 0)], info


def sytrd_team(A, nteam):
    """PDSYTRD('L') on a 1 x P grid, 128-wide column blocks (ek_hip_sytrd_team).  nteam >= 1: the
    whole team rehearsed in this process on one GPU; nteam == 0: this process is one rank of the
    attached communicator.  Returns (A_reflectors, d, e, tau, info, mismatch)."""
    lib = load_library()
    A = np.array(_farr(A), order="F", copy=True)
    n = A.shape[0]
    d = np.zeros(max(n, 1)); e = np.zeros(max(n, 1)); tau = np.zeros(max(n, 1))
    mm = ctypes.c_longlong(-1)
    info = lib.ek_hip_sytrd_team(n, _P(A), _I(_desc_for(A)), _P(d), _P(e), _P(tau), nteam, ctypes.byref(mm))
    return A, d[:n], e[:max(n - 1, 0)], tau[:max(n - 1, 0)], info, mm.value


def potrf_team(B, nteam):
    """PDPOTRF('L') on a 1 x P grid (ek_hip_potrf_team). Returns (B_with_L_in_lower, info, mismatch)."""
    lib = load_library()
    B = np.array(_farr(B), order="F", copy=True)
    mm = ctypes.c_longlong(-1)
    info = lib.ek_hip_potrf_team(B.shape[0], _P(B), _I(_desc_for(B)), nteam, ctypes.byref(mm))
    return B, info, mm.value


def sygst_team(A, L, nteam):
    """PDSYGST(1,'L') on a 1 x P grid (ek_hip_sygst_team). Returns (reduced A, info)."""
    lib = load_library()
    A = np.array(_farr(A), order="F", copy=True)
    L = _farr(L)
    n = A.shape[0]
    info = lib.ek_hip_sygst_team(n, _P(A), _I(_desc_for(A)), _P(L), _I(_desc_for(L)), nteam)
    return A, info


def comm_unique_id():
    """128-byte RCCL id (rank 0 calls this, the host broadcasts it)."""
    lib = load_library()
    buf = ctypes.create_string_buffer(128)
    rc = lib.ek_hip_comm_unique_id(buf, 128)
    if rc:
        raise SolverError("ek_hip_comm_unique_id: %d" % rc, rc)
    return buf.raw


def comm_init(uid, nranks, rank):
    """Attach the RCCL communicator of the distributed path (include/ek_hip.h)."""
    lib = load_library()
    buf = ctypes.create_string_buffer(bytes(uid), 128)
    rc = lib.ek_hip_comm_init(buf, 128, nranks, rank)
    if rc:
        raise SolverError("ek_hip_comm_init: %d" % rc, rc)


def comm_attach_host(nranks, rank):
    """Distributed stages with the exchanges going through the registered allgatherv hook."""
    rc = load_library().ek_hip_comm_attach_host(nranks, rank)
    if rc:
        raise SolverError("ek_hip_comm_attach_host: %d" % rc, rc)


def comm_destroy():
    load_library().ek_hip_comm_destroy()


def stedc(d, e):
    """PDSTEDC('I') (solver_scalapack_all.f90:96). Returns (w, Z, info)."""
    lib = load_library()
    d = np.array(d, dtype=np.float64, copy=True)
    n = d.shape[0]
    ee = np.zeros(max(n, 1)); ee[:max(n - 1, 0)] = np.asarray(e, dtype=np.float64)[:max(n - 1, 0)]
    Z = np.zeros((n, n), order="F")
    info = lib.ek_hip_stedc(n, _P(d), _P(ee), _P(Z), _I(_desc_for(Z)))
    return d, Z, info


def stedc_select(d, e, nsel=-1, first=0, nb=None, npcol=1, mycol=0):
    """The divide & conquer stage in every storage form (ek_hip_debug_stedc): nsel < 0 the full form; otherwise the
    eigenvectors of ranks first + ((l // nb) * npcol + mycol) * nb + l % nb, l = 0..nsel-1 (nb=None: n, a window on a 1x1
    grid).  Returns (w, Z, info, merges): all n eigenvalues, the n x (n or nsel) columns the form produces, the stage's
    info and an (nmerge, 6) int array of {off, n1, n, k, nrot, k1} per merge, the top merge last (k1 = -1 where nrot > 0).
    Raises SolverError on an argument or runtime error."""
    lib = load_library()
    d = np.ascontiguousarray(d, dtype=np.float64)
    n = d.shape[0]
    ee = np.zeros(max(n, 1)); ee[:max(n - 1, 0)] = np.asarray(e, dtype=np.float64)[:max(n - 1, 0)]
    nsel = int(nsel)
    nb = max(n, 1) if nb is None else int(nb)
    ncols = n if nsel < 0 else nsel
    w = np.zeros(max(n, 1))
    Z = np.zeros((max(n, 1), max(ncols, 1)), order="F")
    cap = n // 16 + 2
    merges = np.zeros((cap, 6), dtype=np.int32)
    info = ctypes.c_int(0)
    rc = lib.ek_hip_debug_stedc(n, _P(d), _P(ee), nsel, int(first), nb, int(npcol), int(mycol), _P(w), _P(Z),
                                max(n, 1), _I(merges), cap, ctypes.byref(info))
    if rc < 0:
        raise SolverError("ek_hip_debug_stedc: %d" % rc, rc)
    return w[:n], Z[:n, :max(ncols, 0)], info.value, merges[:rc].copy()


def stedc_zcols(n, nsel=-1):
    """Columns of the n-row array stedc_select gives the stage (ek_hip_debug_stedc_zcols; no GPU): nsel where the stage
    keeps its bases compact, n otherwise."""
    return load_library().ek_hip_debug_stedc_zcols(int(n), int(nsel))


def stebz(d, e, il=1, iu=None):
    """DSTEBZ('I', 'E') on the GPU (ek_hip_stebz): eigenvalues il..iu (1-based, ascending) of the symmetric tridiagonal
    (d, e).  Returns w (iu - il + 1 values); raises SolverError on a nonzero info."""
    lib = load_library()
    d = np.ascontiguousarray(d, dtype=np.float64)
    n = d.shape[0]
    iu = n if iu is None else int(iu)
    ee = np.zeros(max(n, 1)); ee[:max(n - 1, 0)] = np.asarray(e, dtype=np.float64)[:max(n - 1, 0)]
    w = np.zeros(max(iu - int(il) + 1, 1))
    info = lib.ek_hip_stebz(n, _P(d) if n else None, _P(ee), int(il), iu, _P(w))
    if info != 0:
        raise SolverError("ek_hip_stebz failed", info)
    return w[:max(iu - int(il) + 1, 0)] if n else w[:0]


def stebz_range(d, e, vl, vu):
    """DSTEBZ('V', 'E') on the GPU (ek_hip_stebz_range): the eigenvalues of the symmetric tridiagonal (d, e) in
    (vl, vu].  Returns (w, il): w ascending (bit-identical to stebz(d, e, il, il + len(w) - 1)), il the 1-based index of
    the first.  Raises SolverError on a nonzero info."""
    lib = load_library()
    d = np.ascontiguousarray(d, dtype=np.float64)
    n = d.shape[0]
    ee = np.zeros(max(n, 1)); ee[:max(n - 1, 0)] = np.asarray(e, dtype=np.float64)[:max(n - 1, 0)]
    w = np.zeros(max(n, 1))
    il, m = ctypes.c_int(0), ctypes.c_int(0)
    info = lib.ek_hip_stebz_range(n, _P(d) if n else None, _P(ee), float(vl), float(vu), ctypes.byref(il),
                                  ctypes.byref(m), _P(w))
    if info != 0:
        raise SolverError("ek_hip_stebz_range failed", info)
    return w[:m.value].copy(), il.value


def ormtr(Ar, tau, Z):
    """PDORMTR('L','L','N') (solver_scalapack_all.f90:115). Returns (QZ, info)."""
    lib = load_library()
    Ar = _farr(Ar)
    Z = np.array(_farr(Z), order="F", copy=True)
    n = Ar.shape[0]
    t = np.zeros(max(n, 1)); t[:max(n - 1, 0)] = np.asarray(tau, dtype=np.float64)[:max(n - 1, 0)]
    info = lib.ek_hip_ormtr(n, Z.shape[1], _P(Ar), _I(_desc_for(Ar)), _P(t), _P(Z), _I(_desc_for(Z)))
    return Z, info


def debug_ormtr(V, tau, Z, ncols_global=0, slab=0):
    """The back-transformation as the whole path reaches it (ek_hip_debug_ormtr): V the explicit n x n reflectors (column
    j = v_j, zero above its unit entry), tau (n - 1); the T factors formed once, then applied to column slabs of `slab`
    columns (<= 0: one call over all), every call with ncols_global (<= 0: the columns of Z).  Returns Q Z; raises
    SolverError on an argument or runtime error."""
    lib = load_library()
    V = _farr(V)
    Z = np.array(_farr(Z), order="F", copy=True)
    n = V.shape[0]
    t = np.zeros(max(n, 1)); t[:max(n - 1, 0)] = np.asarray(tau, dtype=np.float64)[:max(n - 1, 0)]
    rc = lib.ek_hip_debug_ormtr(n, Z.shape[1], _P(V), max(n, 1), _P(t), _P(Z), max(n, 1), int(ncols_global), int(slab))
    if rc:
        raise SolverError("ek_hip_debug_ormtr: %d" % rc, rc)
    return Z


def trtrs(L, Z):
    """PDTRTRS('L','T','N') (generalized_to_standard.f90:103). Returns (X, info)."""
    lib = load_library()
    L = _farr(L)
    Z = np.array(_farr(Z), order="F", copy=True)
    info = lib.ek_hip_trtrs(L.shape[0], Z.shape[1], _P(L), _I(_desc_for(L)), _P(Z), _I(_desc_for(Z)))
    return Z, info


def sygst_ibtype(A, L, ibtype):
    """PDSYGST(ibtype,'L') (ek_hip_sygst_ibtype): ibtype 1 A <- L^-1 A L^-T, 2 and 3 A <- L^T A L (lower triangles).
    Returns (A_out, info)."""
    lib = load_library()
    A = np.array(_farr(A), order="F", copy=True)
    L = _farr(L)
    scale = ctypes.c_double(0.0)
    info = lib.ek_hip_sygst_ibtype(int(ibtype), A.shape[0], _P(A), _I(_desc_for(A)), _P(L), _I(_desc_for(L)),
                                   ctypes.byref(scale))
    return A, info


def trmm(L, Z):
    """PDTRMM('L','L','N','N') (ek_hip_trmm): Z <- L Z, the recovery of itype 3. Returns (X, info)."""
    lib = load_library()
    L = _farr(L)
    Z = np.array(_farr(Z), order="F", copy=True)
    info = lib.ek_hip_trmm(L.shape[0], Z.shape[1], _P(L), _I(_desc_for(L)), _P(Z), _I(_desc_for(Z)))
    return Z, info


def stage_leaves256(mode):
    """1: sygst, sygst_ibtype(.., 1) and trtrs solve through the 256-block inverses for n >= 256, as the whole path does;
    0: the default (ek_hip_debug_stage_leaves256).  Returns the previous mode."""
    return int(load_library().ek_hip_debug_stage_leaves256(int(mode)))


def set_sygst_direct(order=0):
    """Order at or below which the reductions reduce a block directly (ek_hip_debug_set_sygst_direct): <= 0 restores the
    default of 4096, values below 256 are raised to 256.  Returns the previous order."""
    return int(load_library().ek_hip_debug_set_sygst_direct(int(order)))


def sygst_scratch(n):
    """(doubles of scratch a reduction of order n is given, what type 1's recursion takes, what types 2 / 3's takes) at
    the direct order as it stands (ek_hip_debug_sygst_scratch; host arithmetic)."""
    need = (ctypes.c_ulonglong * 2)(0, 0)
    have = load_library().ek_hip_debug_sygst_scratch(int(n), need)
    return int(have), int(need[0]), int(need[1])


BAND_W = 64   # half bandwidth of the two-stage tridiagonalisation (kBandW in csrc/ek_common.h)


def set_two_stage(min_order=-1):
    """Order from which the whole-path calls tridiagonalise in two stages (-1: default, 0: never)."""
    load_library().ek_hip_debug_set_two_stage(int(min_order))


def stedc_team(nranks=0, levels=-1, profile=False):
    """Team form of the divide & conquer's heights below the top merge (ek_stedc.hip StedcTeam).  levels: sharded heights
    (-1: the library's default for the order and team) -- applies to real teams too; nranks >= 2: grid cells solved
    WITHOUT a communicator rehearse a team of that many, rank after rank in this process.  stedc_team() restores the
    defaults."""
    rc = load_library().ek_hip_debug_stedc_team(int(nranks), int(levels), 1 if profile else 0)
    assert rc == 0, rc


def stedc_team_seconds():
    """[the D&C, all ranks' sections, the longest rank's section per height summed] of the last profiled rehearsal."""
    out = (ctypes.c_double * 3)()
    rc = load_library().ek_hip_debug_stedc_team_get(out)
    assert rc == 0, rc
    return [float(x) for x in out]


def last_solve_stats():
    """What the last whole-path call did: [flops of the D&C's merge products, 1 if it stayed on the two-stage path,
    panels of the first stage that took the Householder rescue, 1 if the band short cut was taken, ...]."""
    st = (ctypes.c_double * 8)()
    load_library().ek_hip_debug_last_solve_stats(st, 8)
    return [float(x) for x in st]


def workspace_bytes(problem, n, n_vec=None, nranks=1):
    """Bytes of device workspace one whole-path call asks for (host arithmetic: works without a GPU): returns
    (total, parts) with parts = [one matrix, L + Q1 reflectors, eigenvector columns, X0, X1, rest]."""
    parts = (ctypes.c_ulonglong * 6)()
    tot = load_library().ek_hip_debug_workspace_bytes(int(problem), int(n), int(n if n_vec is None else n_vec), int(nranks), parts)
    return int(tot), [int(x) for x in parts]


def values_workspace_bytes(problem, n):
    """Bytes of device workspace one eigenvalues-only call asks for (host arithmetic: works without a GPU)."""
    return int(load_library().ek_hip_debug_values_workspace_bytes(int(problem), int(n)))


def set_stebz_lanes(lanes=0):
    """Lanes per eigenvalue index of the bisection (1, 2, 4, 8, 16; 0: the default)."""
    rc = load_library().ek_hip_debug_set_stebz(int(lanes))
    assert rc == 0, rc


def eigenvalues(A, B=None, il=1, iu=None, stage_seconds=None):
    """Eigenvalues il..iu (1-based, ascending) of A x = l x, or of A x = l B x with B SPD (ek_hip_eigenvalues: no
    eigenvectors are formed).  A and B are not modified.  stage_seconds: None or a float64 array of EK_HIP_N_STAGES
    entries that receives the stage times.  Returns w; raises SolverError on a nonzero info."""
    lib = load_library()
    A = _farr(A)
    n = A.shape[0]
    problem = 0 if B is None else 1
    Bf = _farr(B) if B is not None else None
    iu = n if iu is None else int(iu)
    w = np.zeros(max(iu - int(il) + 1, 1))
    st = None if stage_seconds is None else stage_seconds
    info = lib.ek_hip_eigenvalues(problem, n, int(il), iu, _P(A), max(n, 1), _P(Bf) if Bf is not None else None,
                                  max(n, 1), _P(w), _P(st) if st is not None else None, 0 if st is None else len(st))
    if info != 0:
        raise SolverError("ek_hip_eigenvalues failed", info)
    return w[:max(iu - int(il) + 1, 0)] if n else w[:0]


def window_workspace_bytes(problem, n, vectors=True, by_value=False, m=None):
    """Bytes of device workspace one window call (ek_hip_eigenpairs*) with m pairs asks for (host arithmetic)."""
    m = n if m is None else m
    return int(load_library().ek_hip_debug_window_workspace_bytes(int(problem), int(n), 1 if vectors else 0,
                                                                  1 if by_value else 0, int(m)))


def sygvx_workspace_bytes(itype, n, vectors=True, by_value=False, m=None):
    """Bytes of device workspace one ek_hip_sygvx* call with m pairs asks for (host arithmetic; type 1's for all types)."""
    m = n if m is None else m
    return int(load_library().ek_hip_debug_sygvx_workspace_bytes(int(itype), int(n), 1 if vectors else 0,
                                                                 1 if by_value else 0, int(m)))


def sygvx(A, B, itype=1, il=None, iu=None, vl=None, vu=None, vectors=True, stage_seconds=None):
    """DSYGVX on the GPU (ek_hip_sygvx): itype 1 A x = l B x, 2 A B x = l x, 3 B A x = l x, B SPD.  The window and
    the return value are those of eigenpairs: (w, Z or None, ifirst).  Z is B-orthonormal for types 1 and 2,
    B^-1-orthonormal for type 3.  A and B are not modified.  Raises SolverError on a nonzero info."""
    lib = load_library()
    A = _farr(A)
    Bf = _farr(B)
    n = A.shape[0]
    by_value = vl is not None or vu is not None
    if by_value and (il is not None or iu is not None):
        raise ValueError("give either il / iu or vl / vu")
    rng = 1 if by_value else 0
    vl = -np.inf if vl is None else float(vl)
    vu = np.inf if vu is None else float(vu)
    il = 1 if il is None else int(il)
    iu = n if iu is None else int(iu)
    cap = n if by_value else max(iu - il + 1, 0)
    w = np.zeros(max(cap, 1))
    Z = np.zeros((max(n, 1), max(cap, 1)), order="F") if vectors else None
    m, ifirst = ctypes.c_int(0), ctypes.c_int(0)
    st = stage_seconds
    info = lib.ek_hip_sygvx(int(itype), 1 if vectors else 0, rng, n, vl, vu, il, iu, _P(A), max(n, 1), _P(Bf),
                            max(n, 1), ctypes.byref(m), ctypes.byref(ifirst), _P(w), _P(Z) if vectors else None,
                            max(n, 1), max(cap, 1) if vectors else 0, _P(st) if st is not None else None,
                            0 if st is None else len(st))
    if info != 0:
        raise SolverError("ek_hip_sygvx failed", info)
    k = m.value
    return w[:k].copy(), (Z[:n, :k].copy(order="F") if vectors else None), ifirst.value


def eigenpairs(A, B=None, il=None, iu=None, vl=None, vu=None, vectors=True, stage_seconds=None):
    """A window of eigenpairs of A x = l x, or of A x = l B x with B SPD (ek_hip_eigenpairs; PDSYEVX's RANGE).
    By index: il..iu (1-based; defaults 1 and n).  By value: vl and / or vu given -> the eigenvalues in (vl, vu] (a missing
    bound is -inf / +inf).  vectors=False: eigenvalues only.  A and B are not modified.  Returns (w, Z or None, ifirst):
    w the m eigenvalues ascending, Z (n x m) their eigenvectors, ifirst the 1-based index of the first.  Raises
    SolverError on a nonzero info."""
    lib = load_library()
    A = _farr(A)
    n = A.shape[0]
    problem = 0 if B is None else 1
    Bf = _farr(B) if B is not None else None
    by_value = vl is not None or vu is not None
    if by_value and (il is not None or iu is not None):
        raise ValueError("give either il / iu or vl / vu")
    rng = 1 if by_value else 0
    vl = -np.inf if vl is None else float(vl)
    vu = np.inf if vu is None else float(vu)
    il = 1 if il is None else int(il)
    iu = n if iu is None else int(iu)
    cap = n if by_value else max(iu - il + 1, 0)
    w = np.zeros(max(cap, 1))
    Z = np.zeros((max(n, 1), max(cap, 1)), order="F") if vectors else None
    m, ifirst = ctypes.c_int(0), ctypes.c_int(0)
    st = stage_seconds
    info = lib.ek_hip_eigenpairs(problem, 1 if vectors else 0, rng, n, vl, vu, il, iu, _P(A),
                                 max(n, 1), _P(Bf) if Bf is not None else None, max(n, 1), ctypes.byref(m),
                                 ctypes.byref(ifirst), _P(w), _P(Z) if vectors else None, max(n, 1),
                                 max(cap, 1) if vectors else 0, _P(st) if st is not None else None,
                                 0 if st is None else len(st))
    if info != 0:
        raise SolverError("ek_hip_eigenpairs failed", info)
    k = m.value
    return w[:k].copy(), (Z[:n, :k].copy(order="F") if vectors else None), ifirst.value


BATCH_NMAX = 128   # EK_HIP_BATCH_NMAX


def _uniform_mats(A, B):
    """(batch, n, At, Bt) of A (and B, or None) of shape (batch, n, n): float64 copies that are column-major per problem
    (the transpose of each C-ordered slice); Bt is None without B."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 3 or A.shape[1] != A.shape[2]:
        raise ValueError("A must have shape (batch, n, n)")
    Bt = None
    if B is not None:
        B = np.asarray(B, dtype=np.float64)
        if B.shape != A.shape:
            raise ValueError("B must have the shape of A")
        Bt = np.ascontiguousarray(B.transpose(0, 2, 1))
    return A.shape[0], A.shape[1], np.ascontiguousarray(A.transpose(0, 2, 1)), Bt


def _square_list(As, Bs):
    """(Af, Bf, n, ld) of sequences of square 2-D arrays, a problem per entry: Fortran-ordered float64 copies (Bf is None
    without Bs), the orders and the leading dimensions max(n, 1) as int32."""
    Af = []
    for M in As:
        M = np.asarray(M, dtype=np.float64)
        if M.ndim != 2 or M.shape[0] != M.shape[1]:
            raise ValueError("every A must be a square 2-D array")
        Af.append(np.asfortranarray(M))
    Bf = None
    if Bs is not None:
        Bf = [np.asfortranarray(np.asarray(M, dtype=np.float64)) for M in Bs]
        if len(Bf) != len(Af) or any(Bf[b].shape != Af[b].shape for b in range(len(Af))):
            raise ValueError("Bs must hold one array of A's shape per problem")
    n = np.array([M.shape[0] for M in Af], dtype=np.int32)
    return Af, Bf, n, np.maximum(n, 1).astype(np.int32)


_SPARE = np.zeros(1)


def _table(arrays, need=None):
    """The addresses of a problem's array per entry, None for an empty array -- or, where need[b] says that the library
    asks for an address all the same, that of a spare word (never read: such a problem is skipped or empty)."""
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data if a.size else
                                             (_SPARE.ctypes.data if need is not None and need[b] else None)
                                             for b, a in enumerate(arrays)])


def _batched_call(name, first, A, B, vectors, seconds):
    """ek_hip_eigenpairs_batched / ek_hip_sygv_batched on (batch, n, n) arrays; `first` is the first argument (problem
    or itype)."""
    lib = load_library()
    batch, n, At, Bt = _uniform_mats(A, B)
    w = np.zeros((batch, n))
    Zt = np.zeros((batch, n, n)) if vectors else None
    info = np.zeros(max(batch, 1), dtype=np.int32)
    rc = getattr(lib, name)(first, 1 if vectors else 0, n, batch, _P(At), n, n * n,
                            _P(Bt) if Bt is not None else None, n, n * n, _P(w),
                            _P(Zt) if vectors else None, n, n * n, _I(info),
                            _P(seconds) if seconds is not None else None)
    if rc != 0:
        raise SolverError(name + " failed", rc)
    return w, (Zt.transpose(0, 2, 1) if vectors else None), info[:batch]


def eigenpairs_batched(A, B=None, vectors=True, seconds=None):
    """Many small problems in one launch (ek_hip_eigenpairs_batched): A (and B, SPD) of shape (batch, n, n) with
    n <= BATCH_NMAX, lower triangles referenced.  Returns (w, Z or None, info): w[b] problem b's eigenvalues ascending,
    Z[b][:, k] the eigenvector of w[b, k] (B-orthonormal with B), info[b] its status (0; k > 0: B[b] not SPD at pivot
    k; -5: NaN / Inf in A[b]) -- the w and Z of a failed problem are unspecified, the others are unaffected.  A and B
    are not modified.  seconds: None or a float64 array of one entry that receives the device time.  Raises SolverError
    only when the call itself fails (illegal argument, HIP error), never for a problem's info."""
    return _batched_call("ek_hip_eigenpairs_batched", 0 if B is None else 1, A, B, vectors, seconds)


def eigenpairs_window_batched(A, B=None, il=None, iu=None, vl=None, vu=None, vectors=True, zcap=None, seconds=None):
    """A window of eigenpairs of every problem of a batch (ek_hip_eigenpairs_window_batched; _batched_call's conventions):
    A (and B, SPD) of shape (batch, n, n), n <= BATCH_NMAX.  By index: il..iu (1-based; defaults 1 and n).  By value: vl
    and / or vu given -> the eigenvalues in (vl, vu] (a missing bound is -inf / +inf).  zcap: columns of Z per problem
    (default: iu - il + 1 by index, n by value).  Returns (w, Z or None, m, info): m[b] the number of pairs of problem b,
    w[b, :m[b]] its values ascending, Z[b][:, k] the vector of w[b, k] (B-orthonormal with B) for k < m[b]; what lies
    behind m[b] is zero.  info[b]: 0; k > 0 B[b] not SPD at pivot k; -5 NaN / Inf in A[b]; -20 more than zcap values in
    the window (m[b] is their number, nothing else of the problem is returned); 100000 + n + 1, 200000 + k: see
    include/ek_hip.h.  A and B are not modified.  Raises SolverError only when the call itself fails."""
    return _window_batched_call("ek_hip_eigenpairs_window_batched", A, B, il, iu, vl, vu, vectors, zcap, seconds)


def _window_batched_call(entry, A, B, il, iu, vl, vu, vectors, zcap, seconds, itype=None):
    """itype None: the eigenpairs entries (argument 1 is problem); 1 / 2 / 3: the sygv entries (argument 1 is itype)."""
    lib = load_library()
    batch, n, At, Bt = _uniform_mats(A, B)
    by_value = vl is not None or vu is not None
    if by_value and (il is not None or iu is not None):
        raise ValueError("give either il / iu or vl / vu")
    vl = -np.inf if vl is None else float(vl)
    vu = np.inf if vu is None else float(vu)
    il = 1 if il is None else int(il)
    iu = n if iu is None else int(iu)
    if zcap is None:
        zcap = n if by_value else max(iu - il + 1, 0)
    zcap = int(zcap)
    w = np.zeros((batch, n))
    zc = max(zcap, 1)
    Zt = np.zeros((batch, zc, max(n, 1))) if vectors else None
    m = np.zeros(max(batch, 1), dtype=np.int32)
    info = np.zeros(max(batch, 1), dtype=np.int32)
    first = (0 if B is None else 1) if itype is None else int(itype)
    rc = getattr(lib, entry)(first, 1 if vectors else 0, 1 if by_value else 0, n, batch, vl, vu, il, iu, _P(At),
                             max(n, 1), max(n * n, 1), _P(Bt) if Bt is not None else None, max(n, 1), max(n * n, 1),
                             _I(m), _P(w), _P(Zt) if vectors else None, max(n, 1), zcap, zc * max(n, 1), _I(info),
                             _P(seconds) if seconds is not None else None)
    if rc != 0:
        raise SolverError(entry + " failed", rc)
    return w, (Zt.transpose(0, 2, 1)[:, :n, :zcap] if vectors else None), m[:batch], info[:batch]


def window_batched_chunk(problems):
    """Problems per launch of eigenpairs_window_batched (ek_hip_debug_window_batched_chunk): 0 restores the default.
    Returns the previous value.  No result depends on it."""
    return int(load_library().ek_hip_debug_window_batched_chunk(int(problems)))


XBATCH_NMAX = 256   # EK_HIP_XBATCH_NMAX


def eigenpairs_xbatched(A, B=None, vectors=True, seconds=None):
    """eigenpairs_batched for orders up to XBATCH_NMAX (ek_hip_eigenpairs_xbatched): the same arguments, returns and
    errors.  Orders up to BATCH_NMAX give eigenpairs_batched's bits; above it a second kernel class keeps each problem's
    matrix in a device workspace instead of LDS.  An order beyond XBATCH_NMAX raises SolverError with info -3."""
    return _batched_call("ek_hip_eigenpairs_xbatched", 0 if B is None else 1, A, B, vectors, seconds)


def xbatched_chunk(problems):
    """Problems per launch of eigenpairs_xbatched above BATCH_NMAX (ek_hip_debug_xbatched_chunk): 0 restores the default.
    Returns the previous value.  No result depends on it."""
    return int(load_library().ek_hip_debug_xbatched_chunk(int(problems)))


def eigenpairs_window_xbatched(A, B=None, il=None, iu=None, vl=None, vu=None, vectors=True, zcap=None, seconds=None):
    """eigenpairs_window_batched for orders up to XBATCH_NMAX (ek_hip_eigenpairs_window_xbatched): the same arguments,
    returns and errors.  Orders up to BATCH_NMAX give eigenpairs_window_batched's bits; above it the kernel class of
    eigenpairs_xbatched runs the same bisection and inverse iteration.  An order beyond XBATCH_NMAX raises SolverError
    with info -4."""
    return _window_batched_call("ek_hip_eigenpairs_window_xbatched", A, B, il, iu, vl, vu, vectors, zcap, seconds)


def window_xbatched_chunk(problems):
    """Problems per launch of eigenpairs_window_xbatched above BATCH_NMAX (ek_hip_debug_window_xbatched_chunk): 0 restores
    the default.  Returns the previous value.  No result depends on it."""
    return int(load_library().ek_hip_debug_window_xbatched_chunk(int(problems)))


def sygv_window_batched(A, B, itype=1, il=None, iu=None, vl=None, vu=None, vectors=True, zcap=None, seconds=None):
    """eigenpairs_window_batched for DSYGV's three problem types (ek_hip_sygv_window_batched): itype 1 A x = l B x,
    2 A B x = l x, 3 B A x = l x, B SPD and always required.  The window, zcap, the returns (w, Z or None, m, info) and
    the errors are those of eigenpairs_window_batched; Z[b][:, :m[b]] is B-orthonormal for types 1 and 2 and
    B^-1-orthonormal for type 3.  itype 1 returns eigenpairs_window_batched's bits; types 2 and 3 return the same w and
    m.  An itype outside 1..3 raises SolverError with info -1."""
    if B is None:
        raise ValueError("B is required")
    return _window_batched_call("ek_hip_sygv_window_batched", A, B, il, iu, vl, vu, vectors, zcap, seconds, itype)


def sygv_window_xbatched(A, B, itype=1, il=None, iu=None, vl=None, vu=None, vectors=True, zcap=None, seconds=None):
    """sygv_window_batched for orders up to XBATCH_NMAX (ek_hip_sygv_window_xbatched): the same arguments, returns and
    errors.  Orders up to BATCH_NMAX give sygv_window_batched's bits; above it the kernel class of sygv_xbatched runs
    the same bisection and inverse iteration.  An order beyond XBATCH_NMAX raises SolverError with info -4."""
    if B is None:
        raise ValueError("B is required")
    return _window_batched_call("ek_hip_sygv_window_xbatched", A, B, il, iu, vl, vu, vectors, zcap, seconds, itype)


def sygv_batched(A, B, itype=1, vectors=True, seconds=None):
    """eigenpairs_batched for DSYGV's three problem types (ek_hip_sygv_batched): itype 1 A x = l B x, 2 A B x = l x,
    3 B A x = l x, B SPD and always required.  Returns and errors are those of eigenpairs_batched; Z[b] is B-orthonormal
    for types 1 and 2 and B^-1-orthonormal for type 3; itype 1 is eigenpairs_batched(A, B) to the bit.  A missing B or an
    itype outside 1 .. 3 raises ValueError before the library is called."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if B is None:
        raise ValueError("B is required")
    return _batched_call("ek_hip_sygv_batched", int(itype), A, B, vectors, seconds)


def sygv_xbatched(A, B, itype=1, vectors=True, seconds=None):
    """sygv_batched for orders up to XBATCH_NMAX (ek_hip_sygv_xbatched): the same arguments, returns and errors.  Orders
    up to BATCH_NMAX give sygv_batched's bits; above it itype 1 is eigenpairs_xbatched(A, B) to the bit and types 2 and 3
    run that kernel class with the reduction and the recovery of the type.  A missing B or an itype outside 1 .. 3
    raises ValueError before the library is called; an order beyond XBATCH_NMAX raises SolverError with info -3."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if B is None:
        raise ValueError("B is required")
    return _batched_call("ek_hip_sygv_xbatched", int(itype), A, B, vectors, seconds)


YBATCH_NMAX = 512   # EK_HIP_YBATCH_NMAX


def eigenpairs_ybatched(A, B=None, vectors=True, seconds=None):
    """eigenpairs_xbatched for orders up to YBATCH_NMAX (ek_hip_eigenpairs_ybatched): the same arguments, returns and
    errors.  Orders up to XBATCH_NMAX give eigenpairs_xbatched's bits; above it a class of 512 rows of the same kernel
    runs, 256 problems a launch.  An order beyond YBATCH_NMAX raises SolverError with info -3."""
    return _batched_call("ek_hip_eigenpairs_ybatched", 0 if B is None else 1, A, B, vectors, seconds)


def sygv_ybatched(A, B, itype=1, vectors=True, seconds=None):
    """sygv_xbatched for orders up to YBATCH_NMAX (ek_hip_sygv_ybatched): the same arguments, returns and errors.  Orders
    up to XBATCH_NMAX give sygv_xbatched's bits; above it itype 1 is eigenpairs_ybatched(A, B) to the bit and types 2 and
    3 run that kernel class with the reduction and the recovery of the type.  A missing B or an itype outside 1 .. 3
    raises ValueError before the library is called; an order beyond YBATCH_NMAX raises SolverError with info -3."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if B is None:
        raise ValueError("B is required")
    return _batched_call("ek_hip_sygv_ybatched", int(itype), A, B, vectors, seconds)


def ybatched_chunk(problems):
    """Problems per launch of eigenpairs_ybatched and sygv_ybatched above XBATCH_NMAX (ek_hip_debug_ybatched_chunk): 0
    restores the default of 256.  Returns the previous value.  No result depends on it."""
    return int(load_library().ek_hip_debug_ybatched_chunk(int(problems)))


def _vbatched_call(name, first, As, Bs, vectors, seconds):
    """ek_hip_eigenpairs_vbatched / ek_hip_sygv_vbatched on sequences of square arrays; `first` is the first argument
    (problem or itype)."""
    lib = load_library()
    Af, Bf, n, ld = _square_list(As, Bs)
    batch = len(Af)
    if batch == 0:
        return [], ([] if vectors else None), np.zeros(0, dtype=np.int32)
    w = [np.zeros(k) for k in n]
    Z = [np.zeros((k, k), order="F") for k in n] if vectors else None
    info = np.zeros(batch, dtype=np.int32)
    rc = getattr(lib, name)(first, 1 if vectors else 0, batch, _I(n), _table(Af), _I(ld),
                            _table(Bf) if Bf is not None else None, _I(ld), _table(w),
                            _table(Z) if vectors else None, _I(ld), _I(info),
                            _P(seconds) if seconds is not None else None)
    if rc != 0:
        raise SolverError(name + " failed", rc)
    return w, Z, info


def eigenpairs_vbatched(As, Bs=None, vectors=True, seconds=None):
    """Many small problems of DIFFERENT orders in one call (ek_hip_eigenpairs_vbatched): As (and Bs, SPD) sequences of
    square 2-D arrays, problem b of order As[b].shape[0] <= BATCH_NMAX (0 allowed), lower triangles referenced.
    Returns (list of w, list of Z or None, info) with the meaning of eigenpairs_batched per problem; each problem's
    bits are those of eigenpairs_batched on that pair alone.  As and Bs are not modified.  Raises ValueError for bad
    shapes before the library is called, SolverError only when the call itself fails."""
    return _vbatched_call("ek_hip_eigenpairs_vbatched", 0 if Bs is None else 1, As, Bs, vectors, seconds)


def sygv_vbatched(As, Bs, itype=1, vectors=True, seconds=None):
    """eigenpairs_vbatched for DSYGV's three problem types (ek_hip_sygv_vbatched), itype as in sygv_batched, one value
    for the whole call.  Returns and errors are those of eigenpairs_vbatched; each problem's bits are those of
    sygv_batched on that pair alone.  A missing Bs or an itype outside 1 .. 3 raises ValueError before the library is
    called."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if Bs is None:
        raise ValueError("Bs is required")
    return _vbatched_call("ek_hip_sygv_vbatched", int(itype), As, Bs, vectors, seconds)


def eigenpairs_xvbatched(As, Bs=None, vectors=True, seconds=None):
    """eigenpairs_vbatched for orders up to XBATCH_NMAX (ek_hip_eigenpairs_xvbatched): the same arguments, returns and
    errors.  A problem above BATCH_NMAX has the bits of eigenpairs_xbatched on that pair alone, every other one those of
    eigenpairs_vbatched."""
    return _vbatched_call("ek_hip_eigenpairs_xvbatched", 0 if Bs is None else 1, As, Bs, vectors, seconds)


def sygv_xvbatched(As, Bs, itype=1, vectors=True, seconds=None):
    """sygv_vbatched for orders up to XBATCH_NMAX (ek_hip_sygv_xvbatched): the same arguments, returns and errors; each
    problem's bits are those of sygv_xbatched on that pair alone."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if Bs is None:
        raise ValueError("Bs is required")
    return _vbatched_call("ek_hip_sygv_xvbatched", int(itype), As, Bs, vectors, seconds)


def _window_vbatched_call(entry, first, As, Bs, il, iu, vl, vu, vectors, zcap, seconds):
    """ek_hip_eigenpairs_window_xvbatched / ek_hip_sygv_window_xvbatched on sequences of square arrays; `first` is the
    first argument (problem or itype); il, iu, vl, vu, zcap: None, a scalar for every problem, or a value per problem."""
    lib = load_library()
    Af, Bf, n, ld = _square_list(As, Bs)
    batch = len(Af)
    by_value = vl is not None or vu is not None
    if by_value and (il is not None or iu is not None):
        raise ValueError("give either il / iu or vl / vu")
    if batch == 0:
        return [], ([] if vectors else None), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)

    def per_problem(x, default, dtype):
        if x is None:
            x = default
        x = np.asarray(x, dtype=dtype)
        if x.ndim == 0:
            x = np.full(batch, x, dtype=dtype)
        if x.shape != (batch,):
            raise ValueError("a window argument must be a scalar or hold one value per problem")
        return np.ascontiguousarray(x)

    vl = per_problem(vl, -np.inf, np.float64)
    vu = per_problem(vu, np.inf, np.float64)
    il = per_problem(il, 1, np.int32)
    iu = per_problem(iu, n, np.int32)
    zcap = per_problem(zcap, n if by_value else np.maximum(iu - il + 1, 0), np.int32)
    w = [np.zeros(k) for k in n]
    Z = [np.zeros((n[b], max(int(zcap[b]), 0)), order="F") for b in range(batch)] if vectors else None
    m = np.zeros(batch, dtype=np.int32)
    info = np.zeros(batch, dtype=np.int32)
    rc = getattr(lib, entry)(first, 1 if vectors else 0, 1 if by_value else 0, batch, _I(n), _P(vl), _P(vu), _I(il),
                             _I(iu), _table(Af), _I(ld), _table(Bf) if Bf is not None else None, _I(ld), _I(m), _table(w),
                             _table(Z) if vectors else None, _I(ld), _I(zcap), _I(info),
                             _P(seconds) if seconds is not None else None)
    if rc != 0:
        raise SolverError(entry + " failed", rc)
    keep = [int(m[b]) if info[b] == 0 else 0 for b in range(batch)]
    return ([w[b][:keep[b]] for b in range(batch)],
            [Z[b][:, :keep[b]] for b in range(batch)] if vectors else None, m, info)


def eigenpairs_window_xvbatched(As, Bs=None, il=None, iu=None, vl=None, vu=None, vectors=True, zcap=None, seconds=None):
    """A window of eigenpairs PER PROBLEM for problems of different orders up to XBATCH_NMAX in one call
    (ek_hip_eigenpairs_window_xvbatched): As (and Bs, SPD) sequences of square 2-D arrays as in eigenpairs_xvbatched.  By
    index: il, iu (1-based; a scalar for every problem or one value per problem; defaults 1 and the order).  By value: vl
    and / or vu likewise -> the eigenvalues in (vl[b], vu[b]].  zcap: columns of Z per problem (default: iu - il + 1 by
    index, the order by value).  Returns (list of w, list of Z or None, m, info): w[b] the m[b] values of problem b
    ascending, Z[b] its n[b] x m[b] vectors; both empty where info[b] != 0.  info[b] as in eigenpairs_window_batched
    (-20: m[b] is the count).  Each problem's bits are those of eigenpairs_window_xbatched on that pair and window alone.
    As and Bs are not modified.  Raises ValueError for bad shapes, SolverError only when the call itself fails."""
    return _window_vbatched_call("ek_hip_eigenpairs_window_xvbatched", 0 if Bs is None else 1, As, Bs, il, iu, vl, vu,
                                 vectors, zcap, seconds)


def sygv_window_xvbatched(As, Bs, itype=1, il=None, iu=None, vl=None, vu=None, vectors=True, zcap=None, seconds=None):
    """eigenpairs_window_xvbatched for DSYGV's three problem types (ek_hip_sygv_window_xvbatched), itype one value for the
    whole call; each problem's bits are those of sygv_window_xbatched on that pair and window alone.  An itype outside
    1 .. 3 raises SolverError with info -1."""
    if Bs is None:
        raise ValueError("Bs is required")
    return _window_vbatched_call("ek_hip_sygv_window_xvbatched", int(itype), As, Bs, il, iu, vl, vu, vectors, zcap,
                                 seconds)


def window_xvbatched_budget(nbytes):
    """Bytes of LU workspace a launch of eigenpairs_window_xvbatched may hold (ek_hip_debug_window_xvbatched_budget): 0
    restores the defaults.  Returns the previous value.  No result depends on it."""
    return int(load_library().ek_hip_debug_window_xvbatched_budget(int(nbytes)))


CHECK_NOUT = 4   # EK_HIP_CHECK_NOUT: a_norm, res_ave, res_max, orthogonality


def _check_info(info, batch):
    if info is None:
        return None
    info = np.ascontiguousarray(np.asarray(info), dtype=np.int32)
    if info.shape != (batch,):
        raise ValueError("info must hold one int per problem")
    return info


def _check_batched_call(name, first, A, B, w, Z, info, ipr, seconds):
    """ek_hip_check_batched / ek_hip_check_sygv_batched on (batch, n, n) arrays; `first` is the first argument (problem or
    itype)."""
    lib = load_library()
    batch, n, At, Bt = _uniform_mats(A, B)
    Z = np.asarray(Z, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if Z.shape != At.shape:
        raise ValueError("Z must have the shape of A")
    if w.shape != (batch, n):
        raise ValueError("w must have shape (batch, n)")
    info = _check_info(info, batch)
    Zt = np.ascontiguousarray(Z.transpose(0, 2, 1))
    wc = np.ascontiguousarray(w)
    out = np.full((batch, CHECK_NOUT), np.nan)
    q = np.full((batch, n), np.nan) if ipr else None
    if n == 0:                                      # the library references nothing, `out` included
        if batch:
            out[:, 0] = np.where(info != 0, np.nan, 0.0) if info is not None else 0.0
        return out, q
    rc = getattr(lib, name)(first, n, batch, _P(At), n, n * n, _P(Bt) if Bt is not None else None, n, n * n, _P(wc),
                            _P(Zt), n, n * n, _I(info) if info is not None else None, _P(out), _P(q) if ipr else None,
                            _P(seconds) if seconds is not None else None)
    if rc != 0:
        raise SolverError(name + " failed", rc)
    return out, q


def check_batched(A, B, w, Z, info=None, ipr=True, seconds=None):
    """The acceptance checks and the IPRs of every problem of a batch in one launch (ek_hip_check_batched), with the
    normalisations of eigenkernel_amd.verifier: A (and B, or None) of shape (batch, n, n) -- the ORIGINAL matrices, lower
    triangles referenced -- and w (batch, n), Z (batch, n, n) as eigenpairs_batched returns them.  Returns (out, ipr):
    out[b] = (a_norm, res_ave, res_max, orthogonality) of problem b, ipr[b, j] the inverse participation ratio of column
    j (ipr=False: None).  info: None (check every problem) or eigenpairs_batched's status words: a problem with
    info[b] != 0 is skipped, its out row is NaN and its ipr row stays NaN.  seconds: None or a float64 array of one entry
    that receives the device time.  Raises ValueError for bad shapes before the library is called, SolverError only
    when the call itself fails."""
    return _check_batched_call("ek_hip_check_batched", 0 if B is None else 1, A, B, w, Z, info, ipr, seconds)


def check_xbatched(A, B, w, Z, info=None, ipr=True, seconds=None):
    """check_batched for orders up to XBATCH_NMAX (ek_hip_check_xbatched), behind eigenpairs_xbatched: the same arguments
    and returns.  Orders up to BATCH_NMAX run the kernel of check_batched (the same bits); above it a kernel class of its
    own forms A Z, B Z and Z^T B Z on the matrix cores.  An order beyond XBATCH_NMAX raises SolverError with info -2."""
    return _check_batched_call("ek_hip_check_xbatched", 0 if B is None else 1, A, B, w, Z, info, ipr, seconds)


def check_window_xbatched(A, B, m, w, Z, info=None, ipr=True, zcap=None, seconds=None):
    """check_xbatched for a window of eigenpairs per problem (ek_hip_check_window_xbatched), behind
    eigenpairs_window_xbatched, whose m, w, Z and info can be handed over unchanged: A (and B, or None) of shape
    (batch, n, n) -- the ORIGINAL matrices --, m (batch,) ints, w (batch, n) of which w[b, :m[b]] counts, Z (batch, n, zc)
    of which Z[b][:, :m[b]] counts (zcap: None for zc, or a smaller capacity).  Returns (out, ipr) like check_xbatched,
    with the averages over m[b] columns; ipr[b, j] is NaN for j >= m[b].  A problem with info[b] != 0 or m[b] == 0 gets a
    NaN row in both.  Raises ValueError for bad shapes, SolverError when the call itself fails (-10: an m[b] outside
    0 .. n, -14: an m[b] above zcap, of a problem that info does not skip)."""
    return _check_window_call("ek_hip_check_window_xbatched", 0 if B is None else 1, A, B, m, w, Z, info, ipr, zcap, seconds)


def _check_window_call(name, first, A, B, m, w, Z, info, ipr, zcap, seconds):
    """The call behind check_window_xbatched and check_sygv_window_xbatched: `first` is the entry's first argument."""
    lib = load_library()
    batch, n, At, Bt = _uniform_mats(A, B)
    Z = np.asarray(Z, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if Z.ndim != 3 or Z.shape[:2] != (batch, n):
        raise ValueError("Z must have shape (batch, n, columns)")
    if w.shape != (batch, n):
        raise ValueError("w must have shape (batch, n)")
    m = np.ascontiguousarray(np.asarray(m), dtype=np.int32)
    if m.shape != (batch,):
        raise ValueError("m must hold one int per problem")
    zc = Z.shape[2]
    zcap = zc if zcap is None else int(zcap)
    if zcap > zc:
        raise ValueError("zcap exceeds the columns of Z")
    info = _check_info(info, batch)
    Zt = np.ascontiguousarray(Z.transpose(0, 2, 1))
    wc = np.ascontiguousarray(w)
    out = np.full((batch, CHECK_NOUT), np.nan)
    q = np.full((batch, n), np.nan) if ipr else None
    if n == 0 or batch == 0:                        # the library references nothing, `out` included
        return out, q
    rc = getattr(lib, name)(first, n, batch, _P(At), n, n * n, _P(Bt) if Bt is not None else None, n,
                            n * n, _I(m), _P(wc), _P(Zt), n, zcap, max(zc, 1) * n,
                            _I(info) if info is not None else None, _P(out), _P(q) if ipr else None,
                            _P(seconds) if seconds is not None else None)
    if rc != 0:
        raise SolverError(name + " failed", rc)
    return out, q


def check_sygv_window_xbatched(A, B, m, w, Z, itype=1, info=None, ipr=True, zcap=None, seconds=None):
    """check_window_xbatched for DSYGV's three problem types (ek_hip_check_sygv_window_xbatched), behind
    sygv_window_xbatched and sygv_window_batched, whose m, w, Z and info can be handed over unchanged: the shapes and the
    returns of check_window_xbatched.  itype 1 is check_window_xbatched(A, B, ...) to the bit; for types 2 and 3 out[b] =
    (||A||_F ||B||_F, res_ave, res_max, orthogonality) and ipr with the quantities of eigenkernel_amd.verifier's *_sygv
    functions on Z[b][:, :m[b]] (a B[b] that is not SPD gives NaN in orthogonality and ipr of type 3).  A missing B or an
    itype outside 1 .. 3 raises ValueError before the library is called."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if B is None:
        raise ValueError("B is required")
    return _check_window_call("ek_hip_check_sygv_window_xbatched", int(itype), A, B, m, w, Z, info, ipr, zcap, seconds)


def check_xbatched_chunk(problems):
    """Checked problems per launch of check_xbatched above BATCH_NMAX (ek_hip_debug_check_xbatched_chunk): 0 restores the
    default.  Returns the previous value.  No result depends on it."""
    return int(load_library().ek_hip_debug_check_xbatched_chunk(int(problems)))


def check_sygv_batched(A, B, w, Z, itype=1, info=None, ipr=True, seconds=None):
    """check_batched for DSYGV's three problem types (ek_hip_check_sygv_batched), behind sygv_batched: itype 1 is
    check_batched(A, B, ...) to the bit; for types 2 and 3 out[b] = (||A||_F ||B||_F, res_ave, res_max, orthogonality) and
    ipr with the quantities of eigenkernel_amd.verifier's *_sygv functions (a B[b] that is not SPD gives NaN in
    orthogonality and ipr of type 3).  A missing B or an itype outside 1 .. 3 raises ValueError before the library is
    called."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if B is None:
        raise ValueError("B is required")
    return _check_batched_call("ek_hip_check_sygv_batched", int(itype), A, B, w, Z, info, ipr, seconds)


def check_sygv_xbatched(A, B, w, Z, itype=1, info=None, ipr=True, seconds=None):
    """check_sygv_batched for orders up to XBATCH_NMAX (ek_hip_check_sygv_xbatched), behind sygv_xbatched: the same
    arguments and returns.  Orders up to BATCH_NMAX run the kernels of check_sygv_batched (the same bits); above it itype 1
    is check_xbatched(A, B, ...) to the bit, and types 2 and 3 run a kernel class of their own with the products on the
    matrix cores (for the same B and Z, orthogonality and ipr of type 2 are type 1's bits).  A missing B or an itype outside
    1 .. 3 raises ValueError before the library is called; an order beyond XBATCH_NMAX raises SolverError with info -2."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if B is None:
        raise ValueError("B is required")
    return _check_batched_call("ek_hip_check_sygv_xbatched", int(itype), A, B, w, Z, info, ipr, seconds)


def _check_vbatched_call(name, first, As, Bs, ws, Zs, info, ipr, seconds):
    """ek_hip_check_vbatched / ek_hip_check_sygv_vbatched on sequences of arrays; `first` is the first argument."""
    lib = load_library()
    Af, Bf, n, ld = _square_list(As, Bs)
    batch = len(Af)
    Zf = [np.asfortranarray(np.asarray(M, dtype=np.float64)) for M in Zs]
    if len(Zf) != batch or any(Zf[b].shape != Af[b].shape for b in range(batch)):
        raise ValueError("Zs must hold one array of A's shape per problem")
    wf = [np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in ws]
    if len(wf) != batch or any(wf[b].shape != (Af[b].shape[0],) for b in range(batch)):
        raise ValueError("ws must hold one vector of A's order per problem")
    info = _check_info(info, batch)
    out = np.full((batch, CHECK_NOUT), np.nan)
    q = [np.full(M.shape[0], np.nan) for M in Af] if ipr else None
    if batch == 0:
        return out, q
    rc = getattr(lib, name)(first, batch, _I(n), _table(Af), _I(ld), _table(Bf) if Bf is not None else None, _I(ld),
                            _table(wf), _table(Zf), _I(ld), _I(info) if info is not None else None, _P(out),
                            _table(q) if ipr else None, _P(seconds) if seconds is not None else None)
    if rc != 0:
        raise SolverError(name + " failed", rc)
    return out, q


def check_vbatched(As, Bs, ws, Zs, info=None, ipr=True, seconds=None):
    """check_batched for problems of DIFFERENT orders (ek_hip_check_vbatched): As, Bs (or None), ws, Zs sequences as
    eigenpairs_vbatched takes and returns them.  Returns (out, list of ipr arrays or None); a problem of order 0 gets
    a_norm = 0 and NaN in its other three slots.  Each problem's bits are those of check_batched on it alone."""
    return _check_vbatched_call("ek_hip_check_vbatched", 0 if Bs is None else 1, As, Bs, ws, Zs, info, ipr, seconds)


def check_sygv_vbatched(As, Bs, ws, Zs, itype=1, info=None, ipr=True, seconds=None):
    """check_sygv_batched for problems of DIFFERENT orders (ek_hip_check_sygv_vbatched), behind sygv_vbatched; arguments
    and returns as check_vbatched, each problem's bits those of check_sygv_batched on it alone."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if Bs is None:
        raise ValueError("Bs is required")
    return _check_vbatched_call("ek_hip_check_sygv_vbatched", int(itype), As, Bs, ws, Zs, info, ipr, seconds)


def check_xvbatched(As, Bs, ws, Zs, info=None, ipr=True, seconds=None):
    """check_vbatched for orders up to XBATCH_NMAX (ek_hip_check_xvbatched), behind eigenpairs_xvbatched: the same
    arguments and returns.  Each problem's bits are those of check_xbatched on it alone; an order beyond XBATCH_NMAX raises
    SolverError with info -3."""
    return _check_vbatched_call("ek_hip_check_xvbatched", 0 if Bs is None else 1, As, Bs, ws, Zs, info, ipr, seconds)


def check_sygv_xvbatched(As, Bs, ws, Zs, itype=1, info=None, ipr=True, seconds=None):
    """check_sygv_vbatched for orders up to XBATCH_NMAX (ek_hip_check_sygv_xvbatched), behind sygv_xvbatched: the same
    arguments and returns, each problem's bits those of check_sygv_xbatched on it alone (itype 1 is check_xvbatched(As,
    Bs, ...) to the bit)."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if Bs is None:
        raise ValueError("Bs is required")
    return _check_vbatched_call("ek_hip_check_sygv_xvbatched", int(itype), As, Bs, ws, Zs, info, ipr, seconds)


def _check_window_vbatched_call(name, first, As, Bs, m, ws, Zs, info, ipr, zcap, seconds):
    """ek_hip_check_window_xvbatched / ek_hip_check_sygv_window_xvbatched on sequences of arrays; `first` is the first
    argument.  ws[b] and Zs[b] may be shorter than the order: what eigenpairs_window_xvbatched returns."""
    lib = load_library()
    Af, Bf, n, ld = _square_list(As, Bs)
    batch = len(Af)
    Zf = [np.asfortranarray(np.asarray(M, dtype=np.float64)) for M in Zs]
    if len(Zf) != batch or any(Zf[b].ndim != 2 or Zf[b].shape[0] != Af[b].shape[0] for b in range(batch)):
        raise ValueError("Zs must hold one array with A's rows per problem")
    wf = [np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in ws]
    if len(wf) != batch or any(v.ndim != 1 for v in wf):
        raise ValueError("ws must hold one vector per problem")
    m = np.ascontiguousarray(np.asarray(m), dtype=np.int32)
    if m.shape != (batch,):
        raise ValueError("m must hold one int per problem")
    info = _check_info(info, batch)
    cols = np.array([M.shape[1] for M in Zf], dtype=np.int32)
    if zcap is None:
        zcap = cols
    else:
        zcap = np.asarray(zcap, dtype=np.int32)
        zcap = np.full(batch, zcap, dtype=np.int32) if zcap.ndim == 0 else np.ascontiguousarray(zcap)
        if zcap.shape != (batch,):
            raise ValueError("zcap must be a scalar or hold one value per problem")
        if (zcap > cols).any():
            raise ValueError("zcap exceeds the columns of Z")
    live = [(info is None or info[b] == 0) for b in range(batch)]
    if any(live[b] and 0 <= m[b] <= zcap[b] and wf[b].shape[0] < m[b] for b in range(batch)):
        raise ValueError("ws[b] must hold at least m[b] values")
    out = np.full((batch, CHECK_NOUT), np.nan)
    q = [np.full(M.shape[0], np.nan) for M in Af] if ipr else None
    if batch == 0:
        return out, q
    # a problem that is checked hands over what it has; an array without an entry still needs an address where the
    # library asks for one (an order > 0): a skipped or empty problem's is never read
    rc = getattr(lib, name)(first, batch, _I(n), _table(Af, n > 0), _I(ld),
                            _table(Bf, n > 0) if Bf is not None else None, _I(ld), _I(m), _table(wf, n > 0),
                            _table(Zf, (n > 0) & (zcap > 0)), _I(ld), _I(zcap), _I(info) if info is not None else None,
                            _P(out), _table(q) if ipr else None, _P(seconds) if seconds is not None else None)
    if rc != 0:
        raise SolverError(name + " failed", rc)
    return out, q


def check_window_xvbatched(As, Bs, m, ws, Zs, info=None, ipr=True, zcap=None, seconds=None):
    """check_window_xbatched for problems of DIFFERENT orders up to XBATCH_NMAX (ek_hip_check_window_xvbatched), behind
    eigenpairs_window_xvbatched: As, Bs (or None) the ORIGINAL matrices, and m, ws, Zs, info as that function returns
    them -- ws[b] holds at least m[b] values, Zs[b] has n[b] rows and at least m[b] columns (zcap: None for the columns of
    every Zs[b], a scalar or one capacity per problem).  Returns (out, list of ipr arrays or None): out[b] = (a_norm,
    res_ave, res_max, orthogonality) over m[b] columns; ipr[b] has n[b] entries with NaN from m[b] on.  A problem with
    info[b] != 0, m[b] == 0 or order 0 gets a NaN row in both.  Each problem's bits are those of check_window_xbatched on it
    alone.  Raises ValueError for bad shapes, SolverError when the call itself fails (-8: an m[b] outside 0 .. n[b], -12:
    an m[b] above zcap[b], of a problem that info does not skip)."""
    return _check_window_vbatched_call("ek_hip_check_window_xvbatched", 0 if Bs is None else 1, As, Bs, m, ws, Zs, info,
                                       ipr, zcap, seconds)


def check_sygv_window_xvbatched(As, Bs, m, ws, Zs, itype=1, info=None, ipr=True, zcap=None, seconds=None):
    """check_window_xvbatched for DSYGV's three problem types (ek_hip_check_sygv_window_xvbatched), behind
    sygv_window_xvbatched: the same arguments and returns, each problem's bits those of check_sygv_window_xbatched on it
    alone (itype 1 is check_window_xvbatched(As, Bs, ...) to the bit).  A missing Bs or an itype outside 1 .. 3 raises
    ValueError before the library is called."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    if Bs is None:
        raise ValueError("Bs is required")
    return _check_window_vbatched_call("ek_hip_check_sygv_window_xvbatched", int(itype), As, Bs, m, ws, Zs, info, ipr,
                                       zcap, seconds)


def check_xvbatched_last():
    """(seconds, problems) of the classes of 256, 128, 64 and 32 in the last variable-order check call that was given
    `seconds` (ek_hip_debug_check_xvbatched_last)."""
    sec = np.zeros(4)
    cnt = np.zeros(4, dtype=np.int32)
    load_library().ek_hip_debug_check_xvbatched_last(_P(sec), _I(cnt))
    return sec, cnt


def check_sygvx(A, B, w, Z, itype=1):
    """The checks of one problem of any order for DSYGV's three types (ek_hip_check_sygvx), behind sygvx: A, B (n, n) the
    ORIGINAL matrices, w (m,) and Z (n, m) the window's eigenpairs.  Returns the array _check returns for the residual
    with the orthogonality behind it, (norm, res_ave, res_max, orthogonality), and the m IPRs."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    lib = load_library()
    A_, B_, Z_ = _farr(A), _farr(B), _farr(Z)
    n = A_.shape[0]
    if A_.shape != (n, n) or B_.shape != (n, n) or Z_.ndim != 2 or Z_.shape[0] != n or Z_.shape[1] > n:
        raise ValueError("A and B must be (n, n) and Z (n, m) with m <= n")
    m = Z_.shape[1]
    wv = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
    if wv.shape != (m,):
        raise ValueError("w must hold one eigenvalue per column of Z")
    out = np.full(CHECK_NOUT, np.nan)
    q = np.full(m, np.nan)
    ld = max(n, 1)
    info = lib.ek_hip_check_sygvx(int(itype), n, m, _P(A_), ld, _P(B_), ld, _P(wv), _P(Z_), ld, _P(out), _P(q))
    if info:
        raise RuntimeError("ek_hip_check_sygvx info=%d" % info)
    return out, q


def sy2sb(A):
    """Stage 1 of the two-stage tridiagonalisation on its own (include/ek_hip_debug.h):
    returns (A_out with the band in its lower band, V explicit reflectors, tau, flag)."""
    lib = load_library()
    A = np.array(_farr(A), order="F", copy=True)
    n = A.shape[0]
    V = np.zeros((n, n), order="F"); tau = np.zeros(max(n, 1)); flag = ctypes.c_int(-1)
    rc = lib.ek_hip_debug_sy2sb(n, _P(A), max(1, n), _P(V), max(1, n), _P(tau), ctypes.byref(flag))
    if rc:
        raise RuntimeError("ek_hip_debug_sy2sb info=%d" % rc)
    return A, V, tau[:n], flag.value


def sy2sb_stage(A, poison=False):
    """sy2sb through ek_hip_debug_sy2sb_stage; poison: the stage's workspace holds the NaN 0x7FF8DEADBEEF1234 on entry, so
    anything the stage reads of it before writing it shows in the output.  Returns (A_out, V, tau, flag)."""
    lib = load_library()
    A = np.array(_farr(A), order="F", copy=True)
    n = A.shape[0]
    V = np.zeros((n, n), order="F"); tau = np.zeros(max(n, 1)); flag = ctypes.c_int(-1)
    rc = lib.ek_hip_debug_sy2sb_stage(n, _P(A), max(1, n), _P(V), max(1, n), _P(tau), 1 if poison else 0, ctypes.byref(flag))
    if rc:
        raise RuntimeError("ek_hip_debug_sy2sb_stage info=%d" % rc)
    return A, V, tau[:n], flag.value


def set_sy2sb_flow(pair_min=-1, lookahead_min=-1):
    """Rows of a trailing matrix from which sy2sb takes its panels in pairs / factors the next panel beside the update: each
    < 0 as its switch says (the default), 0 never.  Holds until set back: callers restore (-1, -1) in try / finally."""
    rc = load_library().ek_hip_debug_set_sy2sb_flow(int(pair_min), int(lookahead_min))
    if rc:
        raise RuntimeError("ek_hip_debug_set_sy2sb_flow info=%d" % rc)


def sy2sb_team(A, nteam):
    """Stage 1 over a team (rehearsed inside this process for nteam >= 1; nteam = 0: one rank of the attached
    communicator): returns (band in the lower band of an otherwise zero matrix, V, tau, flag, mismatch)."""
    lib = load_library()
    A = np.array(_farr(A), order="F", copy=True)
    n = A.shape[0]
    V = np.zeros((n, n), order="F"); tau = np.zeros(max(n, 1)); flag = ctypes.c_int(-1); mism = ctypes.c_longlong(-1)
    rc = lib.ek_hip_debug_sy2sb_team(n, _P(A), max(1, n), _P(V), max(1, n), _P(tau), int(nteam), ctypes.byref(flag),
                                     ctypes.byref(mism))
    if rc:
        raise RuntimeError("ek_hip_debug_sy2sb_team info=%d" % rc)
    return A, V, tau[:n], flag.value, mism.value


def sb2st(Bd, Z=None):
    """Stage 2 on its own: the lower band (half bandwidth 64) of Bd -> (d, e, Q2 Z or None, flag)."""
    lib = load_library()
    Bd = np.array(_farr(Bd), order="F", copy=True)
    n = Bd.shape[0]
    d = np.zeros(max(n, 1)); e = np.zeros(max(n, 1)); flag = ctypes.c_int(-1)
    if Z is None:
        rc = lib.ek_hip_debug_sb2st(n, _P(Bd), max(1, n), _P(d), _P(e), None, max(1, n), 0, ctypes.byref(flag))
    else:
        Z = np.array(_farr(Z), order="F", copy=True)
        rc = lib.ek_hip_debug_sb2st(n, _P(Bd), max(1, n), _P(d), _P(e), _P(Z), max(1, n), Z.shape[1], ctypes.byref(flag))
    if rc:
        raise RuntimeError("ek_hip_debug_sb2st info=%d" % rc)
    return d[:n], e[:max(n - 1, 0)], Z, flag.value


def sb2st_stage(Bd, Z=None, form=0, chase_mode=0, reflectors=True, pad=0):
    """Stage 2 with what it leaves behind (ek_hip_debug_sb2st_stage): the lower band of Bd -> a dict with d, e, V2 (n x n:
    reflector (s, k) in rows s+1+64k .. of column s), tau2 ((kmax+1) x max(n-2, 1), entry [k, s]), Z (Q2 Z, or None), ran
    (which chase kernel ran: 1 sweeps through memory, 2 positions in registers, 3 the second after the first gave up, 0
    none) and flag.  form 0: the layout of sb2st; form 1: the workspace, packed band and lent records of a whole-path
    solve.  pad > 0: every host array gets that many more rows than it needs, filled with NaN (never to be read).
    reflectors=False: V2 and tau2 are not asked for.  Raises SolverError on an argument or runtime error."""
    lib = load_library()
    Bd = _farr(Bd)
    n = Bd.shape[0]
    pad = int(pad)

    def padded(rows, cols, src=None):
        M = np.full((rows + pad, max(cols, 1)), np.nan, order="F")
        M[:rows] = 0.0 if src is None else src
        return M

    A = padded(n, n, Bd)
    kmax = max(n - 3, 0) // 64 + 1
    d = np.zeros(max(n, 1)); e = np.zeros(max(n, 1)); flag = ctypes.c_int(-1); ran = ctypes.c_int(-1)
    V2 = padded(n, n) if reflectors else None
    tau2 = padded(kmax + 1, max(n - 2, 1)) if reflectors else None
    ncols = 0 if Z is None else _farr(Z).shape[1]
    Zp = padded(n, ncols, _farr(Z)) if ncols > 0 else None
    rc = lib.ek_hip_debug_sb2st_stage(n, _P(A), n + pad, int(form), int(chase_mode), _P(d), _P(e),
                                      _P(V2) if reflectors else None, n + pad, _P(tau2) if reflectors else None,
                                      kmax + 1 + pad, _P(Zp) if ncols > 0 else None, n + pad, ncols, ctypes.byref(ran),
                                      ctypes.byref(flag))
    if rc:
        raise SolverError("ek_hip_debug_sb2st_stage: %d" % rc, rc)
    if pad:
        for M in (A, V2, tau2, Zp):
            if M is not None and not np.isnan(M[M.shape[0] - pad:]).all():
                raise SolverError("ek_hip_debug_sb2st_stage wrote into the padding of a host array", -1)
    def cut(M, rows):
        return None if M is None else np.array(M[:rows], order="F")

    return {"d": d[:n], "e": e[:max(n - 1, 0)], "V2": cut(V2, n), "tau2": cut(tau2, kmax + 1),
            "Z": (cut(Zp, n) if ncols > 0 else (None if Z is None else np.zeros((n, 0)))), "ran": ran.value,
            "flag": flag.value}


def dgemm(transa, transb, alpha, A, B, beta, C, lower_only=False):
    lib = load_library()
    A = _farr(A); B = _farr(B)
    C = np.array(_farr(C), order="F", copy=True)
    m, n = C.shape
    k = A.shape[0] if transa else A.shape[1]
    info = lib.ek_hip_dgemm(int(transa), int(transb), m, n, k, alpha, _P(A), max(1, A.shape[0]),
                            _P(B), max(1, B.shape[0]), beta, _P(C), max(1, m), int(lower_only))
    if info:
        raise RuntimeError("ek_hip_dgemm info=%d" % info)
    return C


# ----------------------------------------------------------------------------- triplet inputs
def _triplets(M):
    """(nnz, suffix, value) of a SparseMat as the C-ABI takes them: suffix interleaved (i_k, j_k) int32 pairs -- the
    memory of the Fortran suffix(2, nnz) -- and float64 values.  The arrays must outlive the call."""
    suf = np.ascontiguousarray(np.asarray(M.suffix, dtype=np.int32).T)
    val = np.ascontiguousarray(M.value, dtype=np.float64)
    if suf.shape != (val.shape[0], 2):
        raise ValueError("SparseMat: suffix must be (2, nnz) and value (nnz,)")
    return int(val.shape[0]), suf, val


def _tp(t):
    nnz, suf, val = t
    return nnz, (_I(suf) if nnz else None), (_P(val) if nnz else None)


def sparse_csr(A):
    """The canonical form the sparse entries work on (ek_hip_debug_sparse_csr; host arithmetic, no GPU): (rowptr, col,
    val) of the CSR of the mirrored matrix, columns 0-based and ascending inside a row, the last of the entries that
    name one unordered pair surviving.  Raises SolverError for an index outside 1 .. n."""
    lib = load_library()
    t = _triplets(A)
    n, nnz = int(A.size), t[0]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    col = np.zeros(max(2 * nnz, 1), dtype=np.int32)
    val = np.zeros(max(2 * nnz, 1))
    m = lib.ek_hip_debug_sparse_csr(n, *_tp(t), rowptr.ctypes.data_as(_llp), _I(col), _P(val))
    if m < 0:
        raise SolverError("ek_hip_debug_sparse_csr failed", int(m))
    return rowptr, col[:m].copy(), val[:m].copy()


def sparse_to_dense(A):
    """The mirrored dense matrix of a SparseMat, densified on the GPU (ek_hip_sparse_to_dense): what the reference's loop
    builds (distribute_matrix.f90:411-418), a later entry replacing an earlier one of the same unordered pair."""
    lib = load_library()
    t = _triplets(A)
    n = int(A.size)
    M = np.zeros((n, n), order="F")
    info = lib.ek_hip_sparse_to_dense(n, *_tp(t), _P(M), max(1, n))
    if info != 0:
        raise SolverError("ek_hip_sparse_to_dense failed", info)
    return M


def solve_sparse(A, B=None, n_vec=None, proc=None, block_size=None):
    """ek_hip_solve_sparse: the whole path on the reference's own arguments, SparseMat A (and B: generalized).  No dense
    matrix is formed on the host; every rank of a grid passes the same triplets and receives its block-cyclic piece of
    the eigenvectors, as with replicated dense inputs.  Returns EigenpairsBlacs; raises SolverError on info != 0."""
    lib = load_library()
    proc = proc or Process()
    n = int(A.size)
    n_vec = n if n_vec is None else int(n_vec)
    ta = _triplets(A)
    tb = _triplets(B) if B is not None else (0, None, None)
    desc_Z, Z_loc = _d.setup_distributed_matrix(n, n, proc.n_procs_row, proc.n_procs_col, proc.my_proc_row,
                                                proc.my_proc_col, block_size=block_size, ctxt=proc.context)
    w = np.zeros(max(n, 1))
    stage = np.zeros(N_STAGES)
    info = lib.ek_hip_solve_sparse(1 if B is not None else 0, n, n_vec, *_tp(ta), *_tp(tb), _P(w), _P(Z_loc),
                                   _I(desc_Z), proc.n_procs_row, proc.n_procs_col, proc.my_proc_row, proc.my_proc_col,
                                   _P(stage), N_STAGES)
    if info != 0:
        raise SolverError("solve_sparse: libek_hip failed", info)
    ep = EigenpairsBlacs(values=w[:n], desc=desc_Z, Vectors=Z_loc, info=info)
    ep.stage_seconds = {lib.ek_hip_stage_name(i).decode(): float(stage[i]) for i in range(N_STAGES)}
    ep.n_vec = n_vec
    return ep


def check_sparse(A, B, w, Z, n_check=None, index1=1, index2=None, n_ipr=None):
    """ek_hip_check_sparse: the reference's acceptance quantities from the triplets of A (and B, None: standard) and
    host arrays w, Z (n x columns).  n_check, index2 and n_ipr default to the columns of Z; n_check = 0, index2 < index1
    or n_ipr = 0 skip a part (its values come back NaN / empty).  Returns (a_norm, res_ave, res_max, orthogonality,
    ipratios)."""
    lib = load_library()
    Z = _farr(Z)
    n, nc = Z.shape
    n_check = nc if n_check is None else int(n_check)
    index2 = nc if index2 is None else int(index2)
    n_ipr = nc if n_ipr is None else int(n_ipr)
    ta = _triplets(A)
    tb = _triplets(B) if B is not None else (0, None, None)
    wv = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
    out = np.full(4, np.nan)
    ipr = np.zeros(max(n_ipr, 1))
    info = lib.ek_hip_check_sparse(1 if B is not None else 0, n, *_tp(ta), *_tp(tb), _P(wv), _P(Z),
                                   max(1, Z.strides[1] // 8 if nc > 1 else n), n_check, int(index1), index2, n_ipr,
                                   _P(out), _P(ipr))
    if info != 0:
        raise SolverError("ek_hip_check_sparse failed", info)
    return float(out[0]), float(out[1]), float(out[2]), float(out[3]), ipr[:max(n_ipr, 0)].copy()


def sparse_check_workspace_bytes(problem, n, nnzA, nnzB=0, n_check=None, index1=1, index2=None, n_ipr=None):
    """Bytes of the cached device workspace one ek_hip_check_sparse_device call asks for (host arithmetic: works without
    a GPU); include/ek_hip_debug.h states the formula."""
    return int(load_library().ek_hip_debug_sparse_check_workspace_bytes(
        int(problem), int(n), int(nnzA), int(nnzB), int(n if n_check is None else n_check), int(index1),
        int(n if index2 is None else index2), int(n if n_ipr is None else n_ipr)))


# ----------------------------------------------------------------------------- the dispatch
def eigen_solver(solver_type, matrix_A, matrix_B=None, n_vec=None, block_size=None, proc=None,
                 inputs="replicated"):
    """eigen_solver (solver_main.f90:22-100) for the hip arms.

    matrix_A / matrix_B: SparseMat (replicated triplets, as the reference passes) or dense
    symmetric ndarrays.  Returns (eigenpairs: EigenpairsBlacs, proc: Process).
    With a process grid larger than 1x1 (proc.n_procs_row x proc.n_procs_col, one rank per GPU)
    every rank passes the same replicated matrices (main.f90:84-86) and receives its
    block-cyclic piece of the eigenvectors (ek_hip_solve_replicated): no collective is issued.
    inputs="distributed" reproduces the reference's own data flow instead: A and B are cut into
    block-cyclic pieces (setup_distributed_matrix + distribute_global_sparse_matrix) and handed
    to ek_hip_solve, which reassembles them through the hook of set_allgatherv().
    inputs="triplets" hands SparseMat matrices on as they are (ek_hip_solve_sparse, on any grid): the dense
    images are built in device memory, the results are those of "replicated" bit for bit.
    Raises SolverError where the reference terminates (info != 0 from the Cholesky,
    reduction or recovery stage), ValueError for an unknown solver
    ('eigen_solver: Unknown solver', solver_main.f90:98).
    """
    if solver_type not in SOLVERS:
        raise ValueError("eigen_solver: Unknown solver %r" % (solver_type,))
    generalized = solver_type.startswith("general_")
    select = solver_type.endswith("_select")
    if generalized and matrix_B is None:
        raise ValueError("eigen_solver: matrix_B is required for %s" % solver_type)
    lib = load_library()
    proc = proc or Process()
    if inputs == "triplets":
        # the reference's own arguments, handed on as they are (ek_hip_solve_sparse): no dense matrix on the host
        if not hasattr(matrix_A, "suffix") or (generalized and not hasattr(matrix_B, "suffix")):
            raise ValueError("eigen_solver: inputs='triplets' takes SparseMat matrices")
        if n_vec is not None and n_vec != matrix_A.size and not select:
            raise ValueError("-n is only legal for *_select solvers (command_argument.f90:186-200)")
        try:
            ep = solve_sparse(matrix_A, matrix_B if generalized else None, n_vec=n_vec if select else None, proc=proc,
                              block_size=block_size)
        except SolverError as e:
            raise SolverError("eigen_solver(%s): libek_hip failed" % solver_type, e.info) from None
        return ep, proc
    gridded = proc.n_procs_row * proc.n_procs_col != 1

    def dense(m):
        return m.to_dense() if hasattr(m, "to_dense") else np.array(_farr(m), order="F", copy=True)

    A = dense(matrix_A)
    n = A.shape[0]
    if n_vec is None or not select:
        if n_vec is not None and n_vec != n and not select:
            raise ValueError("-n is only legal for *_select solvers (command_argument.f90:186-200)")
        n_vec = n if not select or n_vec is None else n_vec
    if gridded and inputs == "distributed":
        g = (proc.n_procs_row, proc.n_procs_col, proc.my_proc_row, proc.my_proc_col)

        def piece(M):
            desc, loc = _d.setup_distributed_matrix(n, n, *g, block_size=block_size, ctxt=proc.context)
            nb = int(desc[_d.BLOCK_ROW_])
            ri = _d.local_indices(n, nb, g[2], g[0]); ci = _d.local_indices(n, nb, g[3], g[1])
            if len(ri) and len(ci):
                loc[:len(ri), :len(ci)] = M[np.ix_(ri, ci)]
            return desc, loc

        desc_A, A_loc = piece(A)
        desc_B, B_loc = piece(dense(matrix_B)) if generalized else (None, None)
        desc_Z, Z_loc = _d.setup_distributed_matrix(n, n, *g, block_size=int(desc_A[_d.BLOCK_ROW_]),
                                                    ctxt=proc.context)
        w = np.zeros(n)
        stage = np.zeros(N_STAGES)
        info = lib.ek_hip_solve(1 if generalized else 0, n, n_vec, _P(A_loc), _I(desc_A),
                                _P(B_loc) if generalized else None,
                                _I(desc_B) if generalized else None, _P(w), _P(Z_loc), _I(desc_Z),
                                *g, _P(stage), N_STAGES)
        if info != 0:
            raise SolverError("eigen_solver(%s): libek_hip failed" % solver_type, info)
        ep = EigenpairsBlacs(values=w, desc=desc_Z, Vectors=Z_loc, info=info)
        ep.stage_seconds = {lib.ek_hip_stage_name(i).decode(): float(stage[i]) for i in range(N_STAGES)}
        ep.n_vec = n_vec
        ep.A_loc, ep.B_loc = A_loc, B_loc
        return ep, proc
    if gridded:
        B = dense(matrix_B) if generalized else None
        desc_Z, Z_loc = _d.setup_distributed_matrix(
            n, n, proc.n_procs_row, proc.n_procs_col, proc.my_proc_row, proc.my_proc_col,
            block_size=block_size, ctxt=proc.context)
        w = np.zeros(n)
        stage = np.zeros(N_STAGES)
        info = lib.ek_hip_solve_replicated(
            1 if generalized else 0, n, n_vec, _P(A), max(1, n), _P(B) if generalized else None,
            max(1, n), _P(w), _P(Z_loc), _I(desc_Z), proc.n_procs_row, proc.n_procs_col,
            proc.my_proc_row, proc.my_proc_col, _P(stage), N_STAGES)
        if info != 0:
            raise SolverError("eigen_solver(%s): libek_hip failed" % solver_type, info)
        ep = EigenpairsBlacs(values=w, desc=desc_Z, Vectors=Z_loc, info=info)
        ep.stage_seconds = {lib.ek_hip_stage_name(i).decode(): float(stage[i]) for i in range(N_STAGES)}
        ep.n_vec = n_vec
        return ep, proc
    # setup_distributed_matrix (distribute_matrix.f90:92-148) on the 1x1 grid
    desc_A, A_loc = _d.setup_distributed_matrix(n, n, block_size=block_size)
    A_loc[:, :] = A
    if generalized:
        desc_B, B_loc = _d.setup_distributed_matrix(n, n, block_size=block_size)
        B_loc[:, :] = dense(matrix_B)
    else:
        desc_B, B_loc = None, None
    desc_Z, Z_loc = _d.setup_distributed_matrix(n, n, block_size=int(desc_A[_d.BLOCK_ROW_]))
    w = np.zeros(n)
    stage = np.zeros(N_STAGES)
    info = lib.ek_hip_solve(1 if generalized else 0, n, n_vec, _P(A_loc), _I(desc_A),
                            _P(B_loc) if generalized else None,
                            _I(desc_B) if generalized else None, _P(w), _P(Z_loc), _I(desc_Z),
                            1, 1, 0, 0, _P(stage), N_STAGES)
    if info != 0:
        raise SolverError("eigen_solver(%s): libek_hip failed" % solver_type, info)
    ep = EigenpairsBlacs(values=w, desc=desc_Z, Vectors=Z_loc, info=info)
    ep.stage_seconds = {lib.ek_hip_stage_name(i).decode(): float(stage[i]) for i in range(N_STAGES)}
    ep.n_vec = n_vec
    return ep, proc
