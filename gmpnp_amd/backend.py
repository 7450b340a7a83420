"""ctypes binding of libgmpnp.so (include/gmpnp.h) — the only way the package computes anything.

There is no CPU fallback: if the HIP library is missing or no GPU is visible, ``DeviceSolver``
raises.  Arrays cross the boundary as contiguous fp64 / int32 / int64 numpy buffers in mesh-file
vertex order (dof = vertex * n_fields + field).
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from ctypes import POINTER, byref, c_double, c_int32, c_int64, c_void_p

import numpy as np

from .model import MAX_SPECIES, CModel, CQuadrature, Model, to_cmodel, to_cquadrature
from .problem import Problem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgmpnp.so")

OK, ERR_INVALID, ERR_HIP, ERR_NOT_CONVERGED, ERR_LINEAR, ERR_NUMERIC = 0, -1, -2, -3, -4, -5
LINEAR_TWOLEVEL, LINEAR_JACOBI, LINEAR_BLOCK_TRIDIAGONAL, LINEAR_BAND_LU = 0, 1, 2, 3
MAX_HISTORY = 64

EXPORTS = [
    "gmpnp_version", "gmpnp_build_id", "gmpnp_last_error", "gmpnp_create", "gmpnp_destroy", "gmpnp_set_model",
    "gmpnp_set_dirichlet", "gmpnp_set_state", "gmpnp_get_state", "gmpnp_assign_previous",
    "gmpnp_newton_solve", "gmpnp_n_fields", "gmpnp_n_dofs", "gmpnp_n_blocks", "gmpnp_jacobian_nnz",
    "gmpnp_n_aggregates", "gmpnp_krylov_launches_per_iteration", "gmpnp_assemble", "gmpnp_get_jacobian_csr", "gmpnp_spmv", "gmpnp_spmv_scaled", "gmpnp_linear_solve",
    "gmpnp_time_kernel", "gmpnp_spmv_profile", "gmpnp_event_overhead",
    "gmpnp_set_supg",
    "gmpnp_create_partition", "gmpnp_comm_unique_id", "gmpnp_comm_create", "gmpnp_comm_selftest", "gmpnp_comm_destroy", "gmpnp_group_create", "gmpnp_group_create_hosted",
    "gmpnp_group_peer_begin", "gmpnp_group_peer_connect",
    "gmpnp_group_destroy", "gmpnp_group_newton_solve", "gmpnp_group_assign_previous", "gmpnp_group_selftest", "gmpnp_group_set_exchange_form", "gmpnp_group_exchange_form", "gmpnp_attach_coarse_level", "gmpnp_group_attach_coarse_group",
    "gmpnp_project_gradient", "gmpnp_project_cellwise", "gmpnp_column_select", "gmpnp_group_column_select",
    "gmpnp_ensemble_create", "gmpnp_ensemble_destroy", "gmpnp_ensemble_size", "gmpnp_ensemble_newton_solve",
    "gmpnp_ensemble_member_error", "gmpnp_ensemble_assign_previous", "gmpnp_ensemble_get_state",
    "gmpnp_ensemble_set_time_step", "gmpnp_ensemble_time_error", "gmpnp_ensemble_time_advance",
    "gmpnp_species_budget", "gmpnp_group_species_budget",
    "gmpnp_step_limit",
    "gmpnp_set_time_step", "gmpnp_time_error", "gmpnp_time_accept", "gmpnp_time_reject",
    "gmpnp_set_time_order", "gmpnp_time_history_levels", "gmpnp_set_time_step_bdf2", "gmpnp_time_error_bdf2", "gmpnp_get_time_history",
    "gmpnp_set_stern", "gmpnp_stern_displacement",
    "gmpnp_set_kinetics", "gmpnp_kinetics_currents",
    "gmpnp_set_galvanostat", "gmpnp_galvanostat_report", "gmpnp_galvanostat_terms",
    "gmpnp_frequency_response",
    "gmpnp_frequency_response_3d", "gmpnp_band_lu_shape",
    "gmpnp_electrode_tangent", "gmpnp_tangent_columns", "gmpnp_electrode_advance",
    "gmpnp_parameter_advance", "gmpnp_get_electrode_options",
    "gmpnp_set_electrode_potential", "gmpnp_electrode_trace_open", "gmpnp_electrode_trace_append", "gmpnp_electrode_trace_read",
    "gmpnp_electrode_trace_close",
    "gmpnp_wall_profile_open", "gmpnp_wall_profile_append", "gmpnp_wall_profile_read", "gmpnp_wall_profile_close",
    "gmpnp_sensitivity_open", "gmpnp_sensitivity_step", "gmpnp_sensitivity_read", "gmpnp_sensitivity_columns", "gmpnp_sensitivity_set_columns",
    "gmpnp_sensitivity_close",
    "gmpnp_cycle_open", "gmpnp_cycle_begin", "gmpnp_cycle_end", "gmpnp_cycle_mix", "gmpnp_cycle_restart", "gmpnp_cycle_vectors",
    "gmpnp_cycle_close",
]
# columns of a species-budget table (gmpnp_budget_column, include/gmpnp.h): per field
#   storage + reaction + wall + exit + point = dirichlet + closure
BUDGET_COLUMNS = ("inventory", "storage", "reaction", "wall", "exit", "point", "dirichlet", "closure")
COMM_ID_BYTES = 128
PEER_HANDLE_BYTES = 64


class CMesh(ctypes.Structure):
    _fields_ = [("dim", c_int32), ("n_vertices", c_int32), ("n_cells", c_int32),
                ("coords", POINTER(c_double)), ("cells", POINTER(c_int32)), ("perm", POINTER(c_int32)),
                ("n_wall_facets", c_int32), ("wall_facets", POINTER(c_int32)),
                ("n_exit_facets", c_int32), ("exit_facets", POINTER(c_int32)),
                ("n_point_vertices", c_int32), ("point_vertices", POINTER(c_int32))]


class CNewtonOptions(ctypes.Structure):
    _fields_ = [("maximum_iterations", c_int32), ("relative_tolerance", c_double),
                ("absolute_tolerance", c_double), ("relaxation_parameter", c_double),
                ("linear_solver", c_int32), ("krylov_relative_tolerance", c_double),
                ("krylov_absolute_tolerance", c_double), ("krylov_maximum_iterations", c_int32),
                ("step_fraction", c_double)]


class CNewtonStats(ctypes.Structure):
    _fields_ = [("iterations", c_int32), ("converged", c_int32), ("krylov_iterations", c_int32),
                ("n_residuals", c_int32), ("residuals", c_double * MAX_HISTORY),
                ("krylov_per_iteration", c_int32 * MAX_HISTORY),
                ("ms_assemble", c_double), ("ms_setup", c_double), ("ms_krylov", c_double), ("ms_total", c_double),
                ("direct_solves", c_int32), ("steric_excursion", c_int32),
                ("limited_steps", c_int32), ("min_step", c_double), ("step_factor", c_double * MAX_HISTORY)]


class CTimeTol(ctypes.Structure):
    """gmpnp_time_tol_t: rtol and one atol per field of the step-size controller's weights."""
    _fields_ = [("rtol", c_double), ("atol", c_double * 9)]


class CTimeError(ctypes.Structure):
    """gmpnp_time_error_t (include/gmpnp.h, adaptive time stepping)."""
    _fields_ = [("err", c_double), ("err_field", c_double * 9), ("rate", c_double), ("rate_field", c_double * 9),
                ("worst_dof", c_int64), ("has_history", c_int32), ("nonfinite", c_int32)]


class CStern(ctypes.Structure):
    """ctypes image of ``gmpnp_stern_t`` (include/gmpnp.h)."""
    _fields_ = [("model", c_int32), ("p_electrode", c_double), ("lam", c_double), ("eps_surface", c_double)]


STERN_MODELS = {"linear": 1, "BDM": 2}   # gmpnp_stern_t.model (0 = off)
MAX_SURFACE_REACTIONS = 4                # GMPNP_MAX_SURFACE_REACTIONS


class CKinetics(ctypes.Structure):
    """ctypes image of ``gmpnp_kinetics_t`` (include/gmpnp.h)."""
    _fields_ = [("n_reactions", c_int32), ("reactant", c_int32 * MAX_SURFACE_REACTIONS), ("k", c_double * MAX_SURFACE_REACTIONS),
                ("alpha", c_double * MAX_SURFACE_REACTIONS), ("p_eq", c_double * MAX_SURFACE_REACTIONS),
                ("nu", (c_double * MAX_SPECIES) * MAX_SURFACE_REACTIONS), ("p_electrode", c_double)]


def to_ckinetics(kin, species) -> CKinetics:
    """The C image of a ``problem.SurfaceKinetics`` record: species names resolved against ``species`` (the model's order)."""
    c = CKinetics()
    c.n_reactions = len(kin.reactions)
    c.p_electrode = float(kin.p_electrode)
    for r, rx in enumerate(kin.reactions):
        c.reactant[r] = -1 if rx.reactant is None else species.index(rx.reactant)
        c.k[r], c.alpha[r], c.p_eq[r] = float(rx.k), float(rx.alpha), float(rx.p_eq)
        for name, v in rx.nu.items():
            c.nu[r][species.index(name)] = float(v)
    return c


class CGalvanostat(ctypes.Structure):
    """ctypes image of ``gmpnp_galvanostat_t`` (include/gmpnp.h)."""
    _fields_ = [("on", c_int32), ("target", c_double), ("weight", c_double * MAX_SURFACE_REACTIONS)]


class CGalvanostatReport(ctypes.Structure):
    """ctypes image of ``gmpnp_galvanostat_report_t`` (include/gmpnp.h)."""
    _fields_ = [("p_electrode", c_double), ("p_electrode_n", c_double), ("I_r", c_double * MAX_SURFACE_REACTIONS), ("I", c_double), ("G", c_double),
                ("cy", c_double), ("cz", c_double), ("d", c_double), ("dp", c_double), ("alpha", c_double)]


class CResponse(ctypes.Structure):
    """ctypes image of ``gmpnp_response_t`` (include/gmpnp.h): C and dI are (re, im) pairs."""
    _fields_ = [("sigma", c_double), ("C", c_double * 2), ("dI", (c_double * 2) * MAX_SURFACE_REACTIONS), ("residual", c_double),
                ("status", c_int32)]


class CTangent(ctypes.Structure):
    """ctypes image of ``gmpnp_tangent_t`` (include/gmpnp.h)."""
    _fields_ = [("param", c_int32), ("dD", c_double), ("dI", c_double * MAX_SURFACE_REACTIONS), ("dp_boundary", c_double),
                ("residual", c_double), ("status", c_int32)]


class CElectrodeRecord(ctypes.Structure):
    """ctypes image of ``gmpnp_electrode_record_t`` (include/gmpnp.h)."""
    _fields_ = [("t", c_double), ("h", c_double), ("p_M", c_double), ("p_boundary", c_double), ("D", c_double), ("dD_dt", c_double),
                ("I", c_double * MAX_SURFACE_REACTIONS), ("Q", c_double * MAX_SURFACE_REACTIONS), ("Q_D", c_double),
                ("u_boundary", c_double * MAX_SPECIES), ("status", c_int32), ("pad_", c_int32)]


ELECTRODE_RECORD_DTYPE = np.dtype([("t", "f8"), ("h", "f8"), ("p_M", "f8"), ("p_boundary", "f8"), ("D", "f8"), ("dD_dt", "f8"),
                                   ("I", "f8", MAX_SURFACE_REACTIONS), ("Q", "f8", MAX_SURFACE_REACTIONS), ("Q_D", "f8"),
                                   ("u_boundary", "f8", MAX_SPECIES), ("status", "i4"), ("pad_", "i4")])
ELECTRODE_RECORD_NONFINITE = 1    # bit of gmpnp_electrode_record_t.status
# image of gmpnp_wall_profile_record_t (include/gmpnp.h "wall profile"): one element per (step, bin)
WALL_PROFILE_RECORD_DTYPE = np.dtype([("t", "f8"), ("h", "f8"), ("z_lo", "f8"), ("z_hi", "f8"), ("area", "f8"), ("D", "f8"),
                                      ("I", "f8", MAX_SURFACE_REACTIONS), ("Q", "f8", MAX_SURFACE_REACTIONS), ("p_mean", "f8"),
                                      ("u_mean", "f8", MAX_SPECIES), ("count", "i4"), ("status", "i4")])
WALL_PROFILE_MAX_BINS = 256       # GMPNP_WALL_PROFILE_MAX_BINS
WALL_PROFILE_NONFINITE = 1        # bit of gmpnp_wall_profile_record_t.status


class CSensitivityRecord(ctypes.Structure):
    """ctypes image of ``gmpnp_sensitivity_record_t`` (include/gmpnp.h)."""
    _fields_ = [("t", c_double), ("h", c_double), ("param", c_int32), ("pad0_", c_int32), ("dD", c_double), ("d_dD_dt", c_double),
                ("dI", c_double * MAX_SURFACE_REACTIONS), ("dQ", c_double * MAX_SURFACE_REACTIONS), ("dQ_D", c_double),
                ("dp_boundary", c_double), ("residual", c_double), ("status", c_int32), ("pad_", c_int32)]


SENSITIVITY_RECORD_DTYPE = np.dtype([("t", "f8"), ("h", "f8"), ("param", "i4"), ("pad0_", "i4"), ("dD", "f8"), ("d_dD_dt", "f8"),
                                     ("dI", "f8", MAX_SURFACE_REACTIONS), ("dQ", "f8", MAX_SURFACE_REACTIONS), ("dQ_D", "f8"),
                                     ("dp_boundary", "f8"), ("residual", "f8"), ("status", "i4"), ("pad_", "i4")])
SENSITIVITY_NONFINITE, SENSITIVITY_SINGULAR, SENSITIVITY_ASSEMBLY = 1, 2, 4   # bits of gmpnp_sensitivity_record_t.status
SENSITIVITY_START = {"zero": 0, "steady": 1, "continue": 2}                  # gmpnp_sensitivity_open's start
TANGENT_MAX_COLUMNS = 10          # GMPNP_TANGENT_MAX_COLUMNS
RESPONSE_MAX_FREQUENCIES = 4096   # gmpnp_frequency_response: n in 1 ... 4096
RESPONSE_SINGULAR, RESPONSE_NONFINITE = 256, 512   # bits of gmpnp_response_t.status


CYCLE_MAX_DEPTH = 8               # GMPNP_CYCLE_MAX_DEPTH


class CCycleReport(ctypes.Structure):
    """ctypes image of ``gmpnp_cycle_report_t`` (include/gmpnp.h, periodic steady state)."""
    _fields_ = [("err", c_double), ("err_max", c_double), ("worst_dof", c_int64), ("n_free", c_int64), ("nonfinite", c_int32),
                ("window", c_int32), ("A", c_double * (CYCLE_MAX_DEPTH * CYCLE_MAX_DEPTH)), ("b", c_double * CYCLE_MAX_DEPTH)]


class CLinearStats(ctypes.Structure):
    _fields_ = [("iterations", c_int32), ("converged", c_int32), ("residual_norm", c_double),
                ("rhs_norm", c_double)]


class COptions(ctypes.Structure):
    """gmpnp_options_t: zero = default for every field (include/gmpnp.h)."""
    _fields_ = [("device_id", c_int32), ("n_aggregates", c_int32), ("shared_device", c_int32),
                ("krylov_batch", c_int32), ("profile_every", c_int32), ("launch_form", c_int32),
                ("warm_start", c_int32), ("coarse_refresh", c_int32), ("progress_by_copy", c_int32),
                ("burst_iterations", c_int32), ("phase_timing", c_int32), ("no_direct_fallback", c_int32),
                ("warm_in_stream", c_int32), ("vector_form", c_int32), ("strict_steric", c_int32), ("element_stores", c_int32), ("band_lu_max_gb", c_double)]


class CPartition(ctypes.Structure):
    """gmpnp_partition_t (include/gmpnp.h)."""
    _fields_ = [("rank", c_int32), ("size", c_int32), ("n_global_aggregates", c_int32),
                ("vertex_aggregate", POINTER(c_int32)), ("vertex_owned", POINTER(ctypes.c_uint8)),
                ("n_neighbours", c_int32), ("neighbour_rank", POINTER(c_int32)),
                ("send_ptr", POINTER(c_int32)), ("send_vertices", POINTER(c_int32)),
                ("recv_ptr", POINTER(c_int32)), ("recv_vertices", POINTER(c_int32))]


ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, c_void_p, POINTER(c_double), c_int32)
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, c_void_p, c_int32, POINTER(c_int32), POINTER(c_int64), POINTER(c_int64), POINTER(c_double),
                               POINTER(c_int64), POINTER(c_int64), POINTER(c_double))


class CHostTransport(ctypes.Structure):
    """gmpnp_host_transport_t (include/gmpnp.h)."""
    _fields_ = [("rank", c_int32), ("size", c_int32), ("allreduce", ALLREDUCE_FN), ("exchange", EXCHANGE_FN), ("user", c_void_p)]


class GmpnpError(RuntimeError):
    """``stats``: what the library had filled into the call's statistics when it failed (``linear_solve``), else None."""

    def __init__(self, code, message, stats=None):
        super().__init__("libgmpnp status %d: %s" % (code, message))
        self.code = code
        self.stats = stats


_lib = None


def load_library(path: str = None):
    """Load libgmpnp.so (built by ``__graft_entry__.build()``).  Fails loudly when it is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("GMPNP_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise RuntimeError("HIP backend %s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % p)
    lib = ctypes.CDLL(p)
    lib.gmpnp_version.restype = ctypes.c_char_p
    lib.gmpnp_last_error.restype = ctypes.c_char_p
    lib.gmpnp_build_id.restype = ctypes.c_char_p
    lib.gmpnp_create.argtypes = [POINTER(CMesh), POINTER(CModel), POINTER(CQuadrature), POINTER(COptions),
                                 POINTER(c_void_p)]
    lib.gmpnp_destroy.argtypes = [c_void_p]
    lib.gmpnp_destroy.restype = None
    lib.gmpnp_set_model.argtypes = [c_void_p, POINTER(CModel)]
    lib.gmpnp_set_dirichlet.argtypes = [c_void_p, c_int64, POINTER(c_int64), POINTER(c_double)]
    lib.gmpnp_set_state.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double)]
    lib.gmpnp_get_state.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double)]
    lib.gmpnp_assign_previous.argtypes = [c_void_p]
    lib.gmpnp_newton_solve.argtypes = [c_void_p, POINTER(CNewtonOptions), POINTER(CNewtonStats)]
    lib.gmpnp_n_fields.argtypes = [c_void_p]
    lib.gmpnp_n_fields.restype = c_int32
    for name in ("gmpnp_n_dofs", "gmpnp_n_blocks", "gmpnp_jacobian_nnz"):
        getattr(lib, name).argtypes = [c_void_p]
        getattr(lib, name).restype = c_int64
    lib.gmpnp_n_aggregates.argtypes = [c_void_p]
    lib.gmpnp_n_aggregates.restype = c_int32
    lib.gmpnp_krylov_launches_per_iteration.argtypes = [c_void_p]
    lib.gmpnp_krylov_launches_per_iteration.restype = c_int32
    lib.gmpnp_assemble.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(c_double)]
    lib.gmpnp_get_jacobian_csr.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_double)]
    lib.gmpnp_spmv.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double)]
    lib.gmpnp_spmv_scaled.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double)]
    lib.gmpnp_linear_solve.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), c_int32, c_double, c_double,
                                       c_int32, POINTER(CLinearStats)]
    lib.gmpnp_set_supg.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int32)]
    lib.gmpnp_time_kernel.argtypes = [c_void_p, c_int32, c_int32, POINTER(c_double)]
    lib.gmpnp_set_time_step.argtypes = [c_void_p, c_double]
    lib.gmpnp_time_error.argtypes = [c_void_p, c_double, c_double, POINTER(CTimeTol), POINTER(CTimeError)]
    lib.gmpnp_time_accept.argtypes = [c_void_p]
    lib.gmpnp_time_reject.argtypes = [c_void_p]
    lib.gmpnp_set_time_order.argtypes = [c_void_p, c_int32]
    lib.gmpnp_time_history_levels.argtypes = [c_void_p, POINTER(c_int32)]
    lib.gmpnp_set_time_step_bdf2.argtypes = [c_void_p, c_double, c_double]
    lib.gmpnp_time_error_bdf2.argtypes = [c_void_p, c_double, c_double, c_double, POINTER(CTimeTol), POINTER(CTimeError)]
    lib.gmpnp_get_time_history.argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_spmv_profile.argtypes = [c_void_p, POINTER(c_int64), POINTER(c_double), POINTER(c_int64)]
    lib.gmpnp_event_overhead.argtypes = [c_void_p, c_int32, POINTER(c_double)]
    lib.gmpnp_create_partition.argtypes = [POINTER(CMesh), POINTER(CModel), POINTER(CQuadrature), POINTER(COptions),
                                           POINTER(CPartition), POINTER(c_void_p)]
    lib.gmpnp_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.gmpnp_comm_create.argtypes = [ctypes.c_char_p, c_int32, c_int32, c_int32, POINTER(c_void_p)]
    lib.gmpnp_comm_destroy.argtypes = [c_void_p]
    lib.gmpnp_comm_selftest.argtypes = [c_void_p, c_int32, POINTER(c_double)]
    lib.gmpnp_comm_destroy.restype = None
    lib.gmpnp_group_create.argtypes = [c_int32, POINTER(c_void_p), c_void_p, POINTER(c_void_p)]
    lib.gmpnp_group_create_hosted.argtypes = [c_void_p, POINTER(CHostTransport), POINTER(c_void_p)]
    lib.gmpnp_group_peer_begin.argtypes = [c_void_p, POINTER(c_void_p), ctypes.c_char_p]
    lib.gmpnp_group_peer_connect.argtypes = [c_void_p, ctypes.c_char_p]
    lib.gmpnp_group_destroy.argtypes = [c_void_p]
    lib.gmpnp_group_destroy.restype = None
    lib.gmpnp_group_newton_solve.argtypes = [c_void_p, POINTER(CNewtonOptions), POINTER(CNewtonStats)]
    lib.gmpnp_group_assign_previous.argtypes = [c_void_p]
    lib.gmpnp_group_selftest.argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_group_set_exchange_form.argtypes = [c_void_p, c_int32]
    lib.gmpnp_group_exchange_form.argtypes = [c_void_p]
    lib.gmpnp_group_exchange_form.restype = c_int32
    lib.gmpnp_attach_coarse_level.argtypes = [c_void_p, c_void_p, POINTER(c_int32), c_double, c_int32]
    lib.gmpnp_group_attach_coarse_group.argtypes = [c_void_p, c_void_p]
    lib.gmpnp_project_gradient.argtypes = [c_void_p, POINTER(c_double), c_double, POINTER(c_double), POINTER(CLinearStats)]
    lib.gmpnp_project_cellwise.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(c_double), POINTER(CLinearStats)]
    for name in ("gmpnp_column_select", "gmpnp_group_column_select"):
        getattr(lib, name).argtypes = [c_void_p, c_int32, POINTER(c_int32), POINTER(c_int64), POINTER(c_double), POINTER(c_int32)]
    lib.gmpnp_ensemble_create.argtypes = [c_int32, POINTER(c_void_p), POINTER(c_void_p)]
    lib.gmpnp_ensemble_destroy.argtypes = [c_void_p]
    lib.gmpnp_ensemble_destroy.restype = None
    lib.gmpnp_ensemble_size.argtypes = [c_void_p]
    lib.gmpnp_ensemble_size.restype = c_int32
    lib.gmpnp_ensemble_newton_solve.argtypes = [c_void_p, POINTER(CNewtonOptions), POINTER(CNewtonStats), POINTER(c_int32)]
    lib.gmpnp_ensemble_member_error.argtypes = [c_void_p, c_int32]
    lib.gmpnp_ensemble_member_error.restype = ctypes.c_char_p
    lib.gmpnp_ensemble_assign_previous.argtypes = [c_void_p]
    lib.gmpnp_ensemble_get_state.argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_ensemble_set_time_step.argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_ensemble_time_error.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(CTimeTol), POINTER(c_int32),
                                              POINTER(CTimeError)]
    lib.gmpnp_ensemble_time_advance.argtypes = [c_void_p, POINTER(c_int32)]
    for name in ("gmpnp_species_budget", "gmpnp_group_species_budget"):
        getattr(lib, name).argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_set_stern.argtypes = [c_void_p, POINTER(CStern)]
    lib.gmpnp_stern_displacement.argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_set_kinetics.argtypes = [c_void_p, POINTER(CKinetics)]
    lib.gmpnp_kinetics_currents.argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_set_galvanostat.argtypes = [c_void_p, POINTER(CGalvanostat)]
    lib.gmpnp_galvanostat_report.argtypes = [c_void_p, POINTER(CGalvanostatReport)]
    lib.gmpnp_galvanostat_terms.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    lib.gmpnp_frequency_response.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(CResponse), POINTER(c_double)]
    lib.gmpnp_frequency_response_3d.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(CResponse), POINTER(c_double)]
    lib.gmpnp_band_lu_shape.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_int32)]
    lib.gmpnp_electrode_tangent.argtypes = [c_void_p, c_int32, POINTER(c_int32), POINTER(CTangent), POINTER(c_double)]
    lib.gmpnp_tangent_columns.argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_electrode_advance.argtypes = [c_void_p, c_double, c_double, POINTER(c_double)]
    lib.gmpnp_parameter_advance.argtypes = [c_void_p, c_int32, POINTER(c_int32), POINTER(c_double), c_double, POINTER(c_double)]
    lib.gmpnp_get_electrode_options.argtypes = [c_void_p, POINTER(CStern), POINTER(CKinetics)]
    lib.gmpnp_set_electrode_potential.argtypes = [c_void_p, c_double]
    lib.gmpnp_electrode_trace_open.argtypes = [c_void_p, c_int32]
    lib.gmpnp_electrode_trace_append.argtypes = [c_void_p, c_double, c_double]
    lib.gmpnp_electrode_trace_read.argtypes = [c_void_p, c_int32, c_int32, POINTER(CElectrodeRecord)]
    lib.gmpnp_electrode_trace_close.argtypes = [c_void_p]
    lib.gmpnp_wall_profile_open.argtypes = [c_void_p, c_int32, POINTER(c_double), c_int32]
    lib.gmpnp_wall_profile_append.argtypes = [c_void_p, c_double, c_double]
    lib.gmpnp_wall_profile_read.argtypes = [c_void_p, c_int32, c_int32, c_void_p]
    lib.gmpnp_wall_profile_close.argtypes = [c_void_p]
    lib.gmpnp_sensitivity_open.argtypes = [c_void_p, c_int32, POINTER(c_int32), c_int32, c_int32]
    lib.gmpnp_sensitivity_step.argtypes = [c_void_p, c_double, c_double]
    lib.gmpnp_sensitivity_read.argtypes = [c_void_p, c_int32, c_int32, POINTER(CSensitivityRecord)]
    lib.gmpnp_sensitivity_columns.argtypes = [c_void_p, c_int32, POINTER(c_double)]
    lib.gmpnp_sensitivity_set_columns.argtypes = [c_void_p, POINTER(c_double)]
    lib.gmpnp_sensitivity_close.argtypes = [c_void_p]
    lib.gmpnp_cycle_open.argtypes = [c_void_p, c_int32, POINTER(CTimeTol)]
    lib.gmpnp_cycle_begin.argtypes = [c_void_p]
    lib.gmpnp_cycle_end.argtypes = [c_void_p, POINTER(CCycleReport)]
    lib.gmpnp_cycle_mix.argtypes = [c_void_p, c_int32, POINTER(c_double), c_double, POINTER(c_double)]
    lib.gmpnp_cycle_restart.argtypes = [c_void_p]
    lib.gmpnp_cycle_vectors.argtypes = [c_void_p, c_int32, POINTER(c_double)]
    lib.gmpnp_cycle_close.argtypes = [c_void_p]
    lib.gmpnp_step_limit.argtypes = [c_void_p, POINTER(c_double), c_double, POINTER(c_double), POINTER(c_double), POINTER(c_int64)]
    if path is None:
        _lib = lib
    return lib


def _dptr(a):
    return a.ctypes.data_as(POINTER(c_double))


def _iptr(a):
    return a.ctypes.data_as(POINTER(c_int32))


def slab_permutation(coords: np.ndarray, cells: np.ndarray, window: int = 224) -> np.ndarray:
    """Internal vertex order handed to ``gmpnp_create`` (``perm[internal] = file``).

    Vertices are sorted along the principal axis of the point cloud (for the pore: z), so contiguous
    ranges are slabs — they become the coarse-space aggregates of the two-level preconditioner and the
    per-GPU partitions.  The library re-sorts by node degree INSIDE each aggregate itself (SELL padding), so the
    default is ``window=0``; a non-zero ``window`` applies that degree sort here in windows of that many vertices."""
    nv = coords.shape[0]
    X = coords - coords.mean(axis=0)
    if coords.shape[1] == 1:
        # interval meshes: plain path order (the block-tridiagonal direct solver needs it)
        return np.argsort(X[:, 0], kind="stable").astype(np.int32)
    else:
        _, vecs = np.linalg.eigh(X.T @ X)
        axis = vecs[:, -1]
        axis = axis * np.sign(axis[np.argmax(np.abs(axis))])
        key = X @ axis
    order = np.argsort(key, kind="stable")
    if not window:
        return order.astype(np.int32)
    k = cells.shape[1]
    pairs = np.unique(np.repeat(cells, k, axis=1).ravel().astype(np.int64) * nv + np.tile(cells, (1, k)).ravel())
    deg = np.bincount((pairs // nv).astype(np.int64), minlength=nv)
    out = order.copy()
    for w0 in range(0, nv, window):
        seg = order[w0:w0 + window]
        out[w0:w0 + window] = seg[np.argsort(-deg[seg], kind="stable")]
    return out.astype(np.int32)


_PC_NOTED = set()


def newton_options(solver_parameters: dict = None, dim: int = 3) -> CNewtonOptions:
    """Translate the reference's ``solver_parameters`` dict (3D:789-798, 1D:357-364) + [3P] DOLFIN
    defaults.  Direct solvers ('default', 'lu', 'mumps', 'umfpack', 'superlu', 'petsc') map to the
    "exact-equivalent" two-level BiCGStab at 1e-10 relative residual (a 3D solve that does not converge falls back
    to the block-banded LU inside the library; ``GMPNP_3D_DIRECT=1`` maps them to that LU from the start, the literal
    reading of 'mumps'); 'band_lu' asks for the LU by name; 'bicgstab' honours ``preconditioner``
    ('jacobi' -> node-block Jacobi; 'default', 'ilu', the AMG names -> two-level, with a warning; 'none' / unknown: refused) and a
    ``krylov_solver`` sub-dict.  ``newton_solver["step_fraction"]`` (an extension key, absent = 0 = off) is the fraction-to-boundary
    step limiter's tau in (0, 1) (gmpnp_newton_options_t.step_fraction, include/gmpnp.h)."""
    sp = dict(solver_parameters or {})
    if sp.get("nonlinear_solver", "newton") != "newton":
        raise RuntimeError("nonlinear_solver %r is not available" % sp.get("nonlinear_solver"))
    ns = dict(sp.get("newton_solver", {}))
    o = CNewtonOptions()
    o.maximum_iterations = int(ns.get("maximum_iterations", 50))
    o.relative_tolerance = float(ns.get("relative_tolerance", 1e-9))
    o.absolute_tolerance = float(ns.get("absolute_tolerance", 1e-10))
    o.relaxation_parameter = float(ns.get("relaxation_parameter", 1.0))
    lin = ns.get("linear_solver", "default")
    ks = dict(ns.get("krylov_solver", {}))
    if lin in ("default", "lu", "mumps", "umfpack", "superlu", "superlu_dist", "petsc"):
        # exact-equivalent modes: 1D -> block-tridiagonal direct solve, 3D -> two-level BiCGStab at 1e-10
        direct3d = os.environ.get("GMPNP_3D_DIRECT", "0") not in ("", "0")
        o.linear_solver = LINEAR_BLOCK_TRIDIAGONAL if dim == 1 else (LINEAR_BAND_LU if direct3d else LINEAR_TWOLEVEL)
        o.krylov_relative_tolerance = float(ks.get("relative_tolerance", 1e-10))
    elif lin in ("band_lu", "gmpnp_band_lu"):
        o.linear_solver = LINEAR_BLOCK_TRIDIAGONAL if dim == 1 else LINEAR_BAND_LU
        o.krylov_relative_tolerance = float(ks.get("relative_tolerance", 1e-10))
    elif lin == "bicgstab":
        # [3P] preconditioner names of the PETSc backend.  Node-block Jacobi is built as such; every name that asks for something
        # stronger than Jacobi (DOLFIN's 'default' = ILU, 'ilu', 'icc', 'sor', the AMG family) gets the one stronger
        # preconditioner this backend has — node-block Jacobi + slab coarse space: a triangular solve per application would
        # serialise the GPU — and says so once; 'none' and unknown names are refused rather than silently replaced.
        pc = ns.get("preconditioner", "default")
        if pc in ("jacobi", "bjacobi"):
            o.linear_solver = LINEAR_JACOBI
        elif pc in ("default", "ilu", "icc", "sor", "amg", "hypre_amg", "petsc_amg", "ml_amg", "hypre_euclid", "hypre_parasails"):
            o.linear_solver = LINEAR_TWOLEVEL
            if pc != "default" and pc not in _PC_NOTED:
                _PC_NOTED.add(pc)
                import warnings
                warnings.warn("preconditioner %r is served by the two-level preconditioner (node-block Jacobi + slab coarse space) "
                              "of the MI355X backend" % pc, stacklevel=2)
        else:
            raise RuntimeError("preconditioner %r is not available in the MI355X backend (jacobi, or default / ilu / amg -> two-level)" % pc)
        o.krylov_relative_tolerance = float(ks.get("relative_tolerance", 1e-6))
    else:
        raise RuntimeError("linear_solver %r is not available in the MI355X backend" % lin)
    o.krylov_absolute_tolerance = float(ks.get("absolute_tolerance", 0.0))
    o.krylov_maximum_iterations = int(ks.get("maximum_iterations", 10000))
    o.step_fraction = float(ns.get("step_fraction", 0.0))
    if o.step_fraction != 0.0 and not 0.0 < o.step_fraction < 1.0:
        raise ValueError("newton_solver['step_fraction'] must be 0 (off) or lie in (0, 1), not %r" % ns.get("step_fraction"))
    return o


def with_step_fraction(solver_parameters: dict, step_fraction: float) -> dict:
    """`solver_parameters` with ``newton_solver["step_fraction"]`` set (a copy); unchanged when `step_fraction` is 0."""
    if not step_fraction:
        return solver_parameters
    sp = dict(solver_parameters or {})
    sp["newton_solver"] = dict(sp.get("newton_solver", {}), step_fraction=float(step_fraction))
    return sp


class DeviceSolver:
    """Device-resident GMPNP problem (one handle = one GPU, one HIP stream)."""

    def __init__(self, problem: Problem, device_id: int = 0, n_aggregates: int = 0, krylov_batch: int = 0,
                 profile_every: int = 0, perm: np.ndarray = None, lib=None, partition: dict = None, **options):
        """``options``: further fields of ``gmpnp_options_t`` by name (shared_device, launch_form, warm_start,
        coarse_refresh, progress_by_copy, burst_iterations, phase_timing, no_direct_fallback, warm_in_stream, vector_form, strict_steric, element_stores,
        band_lu_max_gb); all default to 0."""
        self.lib = lib or load_library()
        self.problem = problem
        self.nf = problem.nf
        self.ndof = problem.ndof
        d = problem.coords.shape[1]
        self._coords = np.ascontiguousarray(problem.coords, dtype=np.float64)
        self._cells = np.ascontiguousarray(problem.cells, dtype=np.int32)
        self.perm = np.ascontiguousarray(
            slab_permutation(self._coords, self._cells, window=0) if perm is None else perm, dtype=np.int32)
        self._wall = np.ascontiguousarray(problem.wall_facets, dtype=np.int32).reshape(-1, 3)
        self._exit = np.ascontiguousarray(problem.exit_facets, dtype=np.int32).reshape(-1, 3)
        self._pts = np.ascontiguousarray(problem.point_vertices, dtype=np.int32)
        m = CMesh()
        m.dim, m.n_vertices, m.n_cells = d, self._coords.shape[0], self._cells.shape[0]
        m.coords, m.cells, m.perm = _dptr(self._coords), _iptr(self._cells), _iptr(self.perm)
        m.n_wall_facets, m.wall_facets = len(self._wall), _iptr(self._wall)
        m.n_exit_facets, m.exit_facets = len(self._exit), _iptr(self._exit)
        m.n_point_vertices, m.point_vertices = len(self._pts), _iptr(self._pts)
        cm, cq = to_cmodel(problem.model), to_cquadrature(problem.quad)
        opts = COptions(device_id=device_id, n_aggregates=n_aggregates, krylov_batch=krylov_batch, profile_every=profile_every)
        known = {f[0] for f in COptions._fields_} - {"reserved_"}
        for k, v in options.items():
            if k not in known:
                raise TypeError("unknown gmpnp_options_t field %r" % k)
            setattr(opts, k, v)
        h = c_void_p()
        self._h = None
        if partition is None:
            self._check(self.lib.gmpnp_create(byref(m), byref(cm), byref(cq), byref(opts), byref(h)))
        else:  # one rank's handle of a mesh-partitioned solve (gmpnp_amd.dist.partition_plan builds the dict)
            keep = {k: np.ascontiguousarray(partition[k], dtype=np.int32) for k in
                    ("vertex_aggregate", "neighbour_rank", "send_ptr", "send_vertices", "recv_ptr", "recv_vertices")}
            keep["vertex_owned"] = np.ascontiguousarray(partition["vertex_owned"], dtype=np.uint8)
            self._partition_arrays = keep
            cp = CPartition()
            cp.rank, cp.size, cp.n_global_aggregates = int(partition["rank"]), int(partition["size"]), int(partition["n_global_aggregates"])
            cp.vertex_aggregate = _iptr(keep["vertex_aggregate"])
            cp.vertex_owned = keep["vertex_owned"].ctypes.data_as(POINTER(ctypes.c_uint8))
            cp.n_neighbours = len(keep["neighbour_rank"])
            cp.neighbour_rank, cp.send_ptr, cp.send_vertices = _iptr(keep["neighbour_rank"]), _iptr(keep["send_ptr"]), _iptr(keep["send_vertices"])
            cp.recv_ptr, cp.recv_vertices = _iptr(keep["recv_ptr"]), _iptr(keep["recv_vertices"])
            self._check(self.lib.gmpnp_create_partition(byref(m), byref(cm), byref(cq), byref(opts), byref(cp), byref(h)))
        self._h = h
        if len(problem.bc_dofs):
            self.set_dirichlet(problem.bc_dofs, problem.bc_vals)
        if getattr(problem, "stern", None) is not None:
            self.set_stern(problem.stern)
        self._n_reactions = 0
        if getattr(problem, "kinetics", None) is not None:
            self.set_kinetics(problem.kinetics)
        if getattr(problem, "galvanostat", None) is not None:
            self.set_galvanostat(problem.galvanostat)

    # ------------------------------------------------------------------------------------------
    def _check(self, code):
        if code != OK:
            raise GmpnpError(code, self.lib.gmpnp_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gmpnp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------------------------------
    @property
    def build_id(self):
        return self.lib.gmpnp_build_id().decode()

    @property
    def n_blocks(self):
        return int(self.lib.gmpnp_n_blocks(self._h))

    @property
    def jacobian_nnz(self):
        return int(self.lib.gmpnp_jacobian_nnz(self._h))

    @property
    def n_aggregates(self):
        return int(self.lib.gmpnp_n_aggregates(self._h))

    @property
    def krylov_launches_per_iteration(self):
        return int(self.lib.gmpnp_krylov_launches_per_iteration(self._h))

    def set_model(self, model: Model):
        cm = to_cmodel(model)
        self._check(self.lib.gmpnp_set_model(self._h, byref(cm)))

    def set_dirichlet(self, dofs, vals):
        dofs = np.ascontiguousarray(dofs, dtype=np.int64)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        if dofs.shape != vals.shape:
            raise ValueError("dofs and values differ in length")
        self._check(self.lib.gmpnp_set_dirichlet(self._h, len(dofs), dofs.ctypes.data_as(POINTER(c_int64)), _dptr(vals)))

    def set_state(self, u=None, un=None):
        pu = pn = None
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64).ravel()
            assert u.size == self.ndof
            pu = _dptr(u)
        if un is not None:
            un = np.ascontiguousarray(un, dtype=np.float64).ravel()
            assert un.size == self.ndof
            pn = _dptr(un)
        self._check(self.lib.gmpnp_set_state(self._h, pu, pn))

    def get_state(self, previous=False):
        out = np.empty(self.ndof)
        if previous:
            self._check(self.lib.gmpnp_get_state(self._h, None, _dptr(out)))
        else:
            self._check(self.lib.gmpnp_get_state(self._h, _dptr(out), None))
        return out

    def assign_previous(self):
        self._check(self.lib.gmpnp_assign_previous(self._h))

    def assemble(self, want_jacobian=True):
        """Returns (b, ||b||_2); the Jacobian stays on the device (``jacobian_csr`` exports it)."""
        F = np.empty(self.ndof)
        norm = c_double()
        self._check(self.lib.gmpnp_assemble(self._h, int(bool(want_jacobian)), _dptr(F), byref(norm)))
        return F, norm.value

    def jacobian_csr(self):
        import scipy.sparse as sp
        nnz = self.jacobian_nnz
        indptr = np.empty(self.ndof + 1, dtype=np.int32)
        indices = np.empty(nnz, dtype=np.int32)
        data = np.empty(nnz)
        self._check(self.lib.gmpnp_get_jacobian_csr(self._h, _iptr(indptr), _iptr(indices), _dptr(data)))
        return sp.csr_matrix((data, indices, indptr), shape=(self.ndof, self.ndof))

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(self.ndof)
        self._check(self.lib.gmpnp_spmv(self._h, _dptr(x), _dptr(y)))
        return y

    def spmv_scaled(self, x):
        """As x with the column-scaled Jacobian of the last preconditioner set-up, read as the Krylov kernels read it."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(self.ndof)
        self._check(self.lib.gmpnp_spmv_scaled(self._h, _dptr(x), _dptr(y)))
        return y

    def linear_solve(self, b, linear_solver=LINEAR_TWOLEVEL, rtol=1e-10, atol=0.0, max_iterations=10000):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.empty(self.ndof)
        st = CLinearStats()
        code = self.lib.gmpnp_linear_solve(self._h, _dptr(b), _dptr(x), linear_solver, rtol, atol, max_iterations, byref(st))
        stats = {"iterations": st.iterations, "converged": bool(st.converged), "residual_norm": st.residual_norm,
                 "rhs_norm": st.rhs_norm}
        if code != OK:   # a solve that stopped at its iteration limit still reports how far it came
            raise GmpnpError(code, self.lib.gmpnp_last_error().decode(), stats)
        return x, stats

    def attach_coarse_level(self, coarse: "DeviceSolver", parents, theta: float = 2.0, sweeps: int = 4):
        """Geometric multilevel term (gmpnp_attach_coarse_level): ``coarse`` = handle of the parent mesh, ``parents`` (nv, 2) the
        two coarse vertices each vertex of this mesh interpolates from (equal: a copy).  The coarse handle is kept alive here."""
        par = np.ascontiguousarray(parents, dtype=np.int32).reshape(-1, 2)
        assert par.shape[0] * self.nf == self.ndof
        self._check(self.lib.gmpnp_attach_coarse_level(self._h, coarse._h, _iptr(par), float(theta), int(sweeps)))
        self._coarse_level = coarse

    def project_gradient(self, f, sign=1.0):
        """``project(sign*grad(f), W).compute_vertex_values()`` for the P1 field with vertex values f (file order): (nv, dim).
        Consistent-mass L2 projection on the device (reference 1D:802-805, 3D:884-909)."""
        f = np.ascontiguousarray(f, dtype=np.float64).ravel()
        nv = self.ndof // self.nf
        assert f.size == nv
        d = self.problem.coords.shape[1]
        out = np.empty((nv, d))
        st = CLinearStats()
        self._check(self.lib.gmpnp_project_gradient(self._h, _dptr(f), float(sign), _dptr(out), byref(st)))
        self.last_projection_iterations = st.iterations
        return out

    def project_cellwise(self, values):
        """``project(f, Y).compute_vertex_values()`` of a cell-wise constant f: values (nc,) or (nc, ncomp <= 4) in file cell order."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        nc = self.problem.cells.shape[0]
        ncomp = 1 if v.ndim == 1 else v.shape[1]
        assert v.size == nc * ncomp
        nv = self.ndof // self.nf
        out = np.empty((nv, ncomp))
        st = CLinearStats()
        self._check(self.lib.gmpnp_project_cellwise(self._h, ncomp, _dptr(v), _dptr(out), byref(st)))
        return out[:, 0] if v.ndim == 1 else out

    def column_select(self, fields, ranks):
        """k-th smallest values of vertex columns of u over this handle's owned rows (gmpnp_column_select): ``fields[j]``,
        ``ranks[j]`` -> (values (n,), nan) with values[j] == np.sort(column fields[j])[ranks[j]] and ``nan`` = some selected column
        holds a NaN (its value is then undefined)."""
        return column_select_call(self.lib.gmpnp_column_select, self._h, fields, ranks, self._check)

    def species_budget(self):
        """(nf, 8) table of this handle's owned rows (gmpnp_species_budget; columns ``BUDGET_COLUMNS``, scaled units of the weak
        form): per field ``storage + reaction + wall + exit + point = dirichlet + closure``; ``dirichlet`` is the consistent flux
        the Dirichlet rows supply, ``closure`` the sum of the residual over the free rows.  Leaves the handle's state untouched."""
        return species_budget_call(self.lib.gmpnp_species_budget, self._h, self.nf, self._check)

    def set_stern(self, stern=None):
        """Stern-layer boundary condition of the potential (``gmpnp_set_stern``): a ``problem.SternLayer`` record, or None = off."""
        c = CStern()
        if stern is not None:
            if stern.model not in STERN_MODELS:
                raise ValueError("Stern model must be one of %s" % sorted(STERN_MODELS))
            c.model, c.p_electrode, c.lam, c.eps_surface = STERN_MODELS[stern.model], float(stern.p_electrode), float(stern.lam), float(stern.eps_surface)
        self._check(self.lib.gmpnp_set_stern(self._h, byref(c)))

    def stern_displacement(self) -> float:
        """The integrated Stern term int g (p_M - p) / lam ds at the current u, in the scaled units of the weak form."""
        out = c_double()
        self._check(self.lib.gmpnp_stern_displacement(self._h, byref(out)))
        return float(out.value)

    def set_kinetics(self, kinetics=None):
        """Potential-dependent surface kinetics on the Stern boundary (``gmpnp_set_kinetics``): a ``problem.SurfaceKinetics`` record
        (species by name, resolved against the problem's model), or None = off."""
        c = CKinetics()
        if kinetics is not None:
            c = to_ckinetics(kinetics, list(self.problem.model.species))
        self._check(self.lib.gmpnp_set_kinetics(self._h, byref(c)))
        self._n_reactions = int(c.n_reactions)

    def kinetics_currents(self) -> np.ndarray:
        """sum_I w_I rate_r at the current u, one entry per reaction (``gmpnp_kinetics_currents``)."""
        out = (c_double * MAX_SURFACE_REACTIONS)()
        self._check(self.lib.gmpnp_kinetics_currents(self._h, out))
        return np.array(out[:self._n_reactions], dtype=np.float64)

    def set_galvanostat(self, galvanostat=None):
        """Galvanostatic mode (``gmpnp_set_galvanostat``): a ``problem.Galvanostat`` record, or None = off (the potential that was
        found stays in the Stern and kinetics options)."""
        c = CGalvanostat()
        if galvanostat is not None:
            c.on, c.target = 1, float(galvanostat.target)
            for r, w in enumerate(galvanostat.weights):
                c.weight[r] = float(w)
        self._check(self.lib.gmpnp_set_galvanostat(self._h, byref(c)))

    def galvanostat_report(self) -> dict:
        """``gmpnp_galvanostat_report``: p_electrode now and at u_n, the currents I_r, I and G at the current u, and the last
        iteration's cy, cz, d, dp, alpha."""
        r = CGalvanostatReport()
        self._check(self.lib.gmpnp_galvanostat_report(self._h, byref(r)))
        out = {k: float(getattr(r, k)) for k in ("p_electrode", "p_electrode_n", "I", "G", "cy", "cz", "d", "dp", "alpha")}
        out["I_r"] = np.array(r.I_r[:self._n_reactions], dtype=np.float64)
        return out

    def galvanostat_terms(self, x=None):
        """``gmpnp_galvanostat_terms`` at the current u and p_M: (b = dF/dp_M in file order, {G, d, I, cx}) with cx = c.x for ``x``
        (file order; None: 0)."""
        b = np.empty(self.ndof)
        sc = (c_double * 4)()
        xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        assert xx is None or xx.size == self.ndof
        self._check(self.lib.gmpnp_galvanostat_terms(self._h, None if xx is None else _dptr(xx), _dptr(b), sc))
        return b, {"G": float(sc[0]), "d": float(sc[1]), "I": float(sc[2]), "cx": float(sc[3])}

    def frequency_response(self, sigmas, want_x=False) -> dict:
        """``gmpnp_frequency_response`` at the current u and p_M: the small-signal response per unit of p_M at the time-term
        multipliers ``sigmas`` (>= 0, i sigma in the place of inv_dt).  Returns sigma (n,), C (n,) complex, dI (n, n_reactions)
        complex, residual (n,), status (n,) and, with ``want_x``, x (n, ndof) complex in file order."""
        return self._frequency_response(self.lib.gmpnp_frequency_response, sigmas, want_x)

    def frequency_response_3d(self, sigmas, want_x=False) -> dict:
        """``gmpnp_frequency_response_3d``: the same response of a 3D handle by the complex block-banded LU; the dictionary of
        ``frequency_response``.  C and dI are sums over the wall (``electrode_tangent``'s dD and dI at sigma = 0, inv_dt = 0)."""
        return self._frequency_response(self.lib.gmpnp_frequency_response_3d, sigmas, want_x)

    def band_lu_shape(self):
        """(node blocks, stored band width) of a 3D handle's block-banded LU (``gmpnp_band_lu_shape``)."""
        n, band = c_int32(), c_int32()
        self._check(self.lib.gmpnp_band_lu_shape(self._h, byref(n), byref(band)))
        return int(n.value), int(band.value)

    def _frequency_response(self, entry, sigmas, want_x) -> dict:
        sg = np.ascontiguousarray(sigmas, dtype=np.float64).ravel()
        n = int(sg.size)
        out = (CResponse * max(n, 1))()
        x = np.empty((n, self.ndof, 2)) if want_x else None
        self._check(entry(self._h, n, _dptr(sg), out, None if x is None else _dptr(x)))
        rec = np.frombuffer(out, dtype=np.dtype([("sigma", "f8"), ("C", "f8", 2), ("dI", "f8", (MAX_SURFACE_REACTIONS, 2)), ("residual", "f8"),
                                                 ("status", "i4"), ("pad", "i4")]), count=n)
        res = {"sigma": rec["sigma"].copy(), "C": rec["C"][:, 0] + 1j * rec["C"][:, 1],
               "dI": (rec["dI"][:, :, 0] + 1j * rec["dI"][:, :, 1])[:, :self._n_reactions], "residual": rec["residual"].copy(),
               "status": rec["status"].copy()}
        if want_x:
            res["x"] = x[:, :, 0] + 1j * x[:, :, 1]
        return res

    def electrode_tangent(self, params, want_z=False) -> dict:
        """``gmpnp_electrode_tangent`` at the current u, p_M and inv_dt: the tangents z_k = du/dtheta_k for the parameter codes
        ``params`` (``polarisation.PARAM_*``).  Returns param (n,), dD (n,), dI (n, n_reactions), dp_boundary (n,), residual (n,),
        status (n,) and, with ``want_z``, z (n, ndof) in file order."""
        pr = np.ascontiguousarray(params, dtype=np.int32).ravel()
        n = int(pr.size)
        out = (CTangent * max(n, 1))()
        z = np.empty((n, self.ndof)) if want_z else None
        self._check(self.lib.gmpnp_electrode_tangent(self._h, n, _iptr(pr), out, None if z is None else _dptr(z)))
        rec = np.frombuffer(out, dtype=np.dtype([("param", "i4"), ("pad0", "i4"), ("dD", "f8"), ("dI", "f8", MAX_SURFACE_REACTIONS),
                                                 ("dp_boundary", "f8"), ("residual", "f8"), ("status", "i4"), ("pad", "i4")]), count=n)
        res = {"param": rec["param"].copy(), "dD": rec["dD"].copy(), "dI": rec["dI"][:, :self._n_reactions].copy(),
               "dp_boundary": rec["dp_boundary"].copy(), "residual": rec["residual"].copy(), "status": rec["status"].copy()}
        if want_z:
            res["z"] = z
        return res

    def tangent_columns(self, n) -> np.ndarray:
        """``gmpnp_tangent_columns``: the columns c_k = dF/dtheta_k of the last ``electrode_tangent`` call of ``n`` columns, (n, ndof)
        in file order."""
        c = np.empty((int(n), self.ndof))
        self._check(self.lib.gmpnp_tangent_columns(self._h, _dptr(c)))
        return c

    def electrode_advance(self, dp, tau=0.0) -> float:
        """``gmpnp_electrode_advance``: p_electrode += dp in the Stern and kinetic options, u += alpha dp z_0 with the p_M tangent of
        the last ``electrode_tangent`` (which must belong to the present state).  Returns alpha (1 with ``tau`` = 0)."""
        alpha = c_double()
        self._check(self.lib.gmpnp_electrode_advance(self._h, float(dp), float(tau), byref(alpha)))
        return float(alpha.value)

    def parameter_advance(self, params, dtheta, tau=0.0) -> float:
        """``gmpnp_parameter_advance``: the parameters ``params`` (codes of the last ``electrode_tangent`` call) move by ``dtheta`` in
        the Stern and kinetic options, u += alpha sum_k dtheta_k z_k.  Returns alpha (1 with ``tau`` = 0)."""
        pr = np.ascontiguousarray(params, dtype=np.int32).ravel()
        dt = np.ascontiguousarray(dtheta, dtype=np.float64).ravel()
        if pr.size != dt.size:
            raise ValueError("parameter advance: %d parameters and %d steps" % (pr.size, dt.size))
        alpha = c_double()
        self._check(self.lib.gmpnp_parameter_advance(self._h, int(pr.size), _iptr(pr), _dptr(dt), float(tau), byref(alpha)))
        return float(alpha.value)

    def electrode_options(self):
        """``gmpnp_get_electrode_options``: (stern, kinetics) as the handle holds them now, each a dict of the fields of
        ``problem.SternLayer`` / ``problem.SurfaceKinetics`` (reactions as dicts of ``problem.SurfaceReaction``'s fields, species by
        name), or None while the option is off."""
        cs, ck = CStern(), CKinetics()
        self._check(self.lib.gmpnp_get_electrode_options(self._h, byref(cs), byref(ck)))
        stern = kinetics = None
        if cs.model != 0:
            model = {v: k for k, v in STERN_MODELS.items()}[int(cs.model)]
            stern = {"model": model, "p_electrode": float(cs.p_electrode), "lam": float(cs.lam), "eps_surface": float(cs.eps_surface)}
        if ck.n_reactions != 0:
            species = list(self.problem.model.species)
            reactions = []
            for r in range(int(ck.n_reactions)):
                nu = {name: float(ck.nu[r][i]) for i, name in enumerate(species) if ck.nu[r][i] != 0.0}
                reactions.append({"k": float(ck.k[r]), "alpha": float(ck.alpha[r]), "p_eq": float(ck.p_eq[r]),
                                  "reactant": None if ck.reactant[r] < 0 else species[ck.reactant[r]], "nu": nu})
            kinetics = {"reactions": reactions, "p_electrode": float(ck.p_electrode)}
        return stern, kinetics

    def set_electrode_potential(self, p):
        """``gmpnp_set_electrode_potential``: p_electrode of the Stern option and, where they are on, of the kinetics becomes ``p`` in
        one call (the bits ``set_stern`` followed by ``set_kinetics`` with that value leave)."""
        self._check(self.lib.gmpnp_set_electrode_potential(self._h, float(p)))

    def _read_records(self, call, dtype, first, n, width=None):
        """Rows ``first`` ... ``first + n - 1`` of a record stream by its read call, as a structured array of ``dtype``: (n,), or
        (n, width) where a row holds ``width`` records."""
        n, w = int(n), 1 if width is None else max(int(width), 1)
        out = np.zeros((max(n, 1), w), dtype=dtype)
        self._check(call(self._h, int(first), n, out.ctypes.data_as(call.argtypes[3])))
        return out[:max(n, 0), 0] if width is None else out[:max(n, 0)]

    def electrode_trace_open(self, capacity):
        """``gmpnp_electrode_trace_open``: a trace of ``capacity`` records; D at the current u becomes D_prev, Q and Q_D start at 0."""
        self._check(self.lib.gmpnp_electrode_trace_open(self._h, int(capacity)))

    def electrode_trace_append(self, t, h):
        """``gmpnp_electrode_trace_append``: the record of the step of length ``h`` that ends at ``t`` with the current u, formed and
        stored on the device (no synchronisation, no copy)."""
        self._check(self.lib.gmpnp_electrode_trace_append(self._h, float(t), float(h)))

    def electrode_trace_read(self, first, n) -> np.ndarray:
        """``gmpnp_electrode_trace_read``: records ``first`` ... ``first + n - 1`` as a structured array (``ELECTRODE_RECORD_DTYPE``;
        I and Q hold ``MAX_SURFACE_REACTIONS`` entries, u_boundary ``MAX_SPECIES``)."""
        return self._read_records(self.lib.gmpnp_electrode_trace_read, ELECTRODE_RECORD_DTYPE, first, n)

    def electrode_trace_close(self):
        """``gmpnp_electrode_trace_close``."""
        self._check(self.lib.gmpnp_electrode_trace_close(self._h))

    # periodic steady state: the accelerated cycle map (include/gmpnp.h "periodic steady state", gmpnp_amd/periodic.py)
    def cycle_open(self, depth, rtol, atol):
        """``gmpnp_cycle_open``: a window of at most ``depth`` + 1 pairs (1 <= depth <= 8) and the weights w = atol_f + rtol |u_n| of
        the CURRENT u_n (``atol``: a scalar or one value per field)."""
        tol = CTimeTol()
        _fill_time_tol(tol, self.nf, rtol, atol)
        self._check(self.lib.gmpnp_cycle_open(self._h, int(depth), byref(tol)))

    def cycle_begin(self):
        """``gmpnp_cycle_begin``: x_k <- u_n."""
        self._check(self.lib.gmpnp_cycle_begin(self._h))

    def cycle_end(self):
        """``gmpnp_cycle_end``: g_k <- u_n; the report as a dict: err, err_max, worst_dof (file order, -1: none), n_free, nonfinite,
        window (pairs, m + 1) and the normal system of the window's m differences, A (m, m) and b (m,)."""
        r = CCycleReport()
        self._check(self.lib.gmpnp_cycle_end(self._h, byref(r)))
        m = max(int(r.window) - 1, 0)
        A = np.array(r.A[:]).reshape(CYCLE_MAX_DEPTH, CYCLE_MAX_DEPTH)[:m, :m].copy()
        return {"err": r.err, "err_max": r.err_max, "worst_dof": int(r.worst_dof), "n_free": int(r.n_free), "nonfinite": bool(r.nonfinite),
                "window": int(r.window), "A": A, "b": np.array(r.b[:m])}

    def cycle_mix(self, gamma, tau: float = 0.0) -> float:
        """``gmpnp_cycle_mix``: u = u_n <- g_k + alpha (sum_j gamma_j g_j - g_k) on the free rows, g_k on the Dirichlet rows; returns
        alpha (1 with ``tau`` = 0, else the step limiter's factor).  Afterwards the handle is where ``set_state(u, u)`` leaves it."""
        g = np.ascontiguousarray(gamma, dtype=np.float64).ravel()
        alpha = c_double()
        self._check(self.lib.gmpnp_cycle_mix(self._h, int(g.size), _dptr(g), float(tau), byref(alpha)))
        return alpha.value

    def cycle_restart(self):
        """``gmpnp_cycle_restart``: empties the window."""
        self._check(self.lib.gmpnp_cycle_restart(self._h))

    def cycle_vectors(self, which, window=None):
        """``gmpnp_cycle_vectors`` (parity hook, file order): ``which`` = "x" or "g": (``window``, ndof) in window order (``window``: the
        pairs held, as the last report said); "w": the weights (ndof,)."""
        code = {"x": 0, "g": 1, "w": 2}[which]
        out = np.empty(self.ndof if code == 2 else (int(window), self.ndof))
        if out.size:
            self._check(self.lib.gmpnp_cycle_vectors(self._h, code, _dptr(out)))
        return out

    def cycle_close(self):
        """``gmpnp_cycle_close``."""
        self._check(self.lib.gmpnp_cycle_close(self._h))

    def wall_profile_open(self, edges, capacity):
        """``gmpnp_wall_profile_open``: the wall of the 3D pore in ``len(edges) - 1`` axial bins with the edges ``edges`` (z, the mesh's
        third coordinate in units of L; ``programme.wall_bin``) and a buffer of ``capacity`` steps; the charges of the bins start at 0."""
        e = np.ascontiguousarray(edges, dtype=np.float64).ravel()
        self._check(self.lib.gmpnp_wall_profile_open(self._h, int(e.size) - 1, e.ctypes.data_as(POINTER(c_double)), int(capacity)))
        self._wall_profile_bins = int(e.size) - 1

    def wall_profile_append(self, t, h):
        """``gmpnp_wall_profile_append``: the records of every bin for the step of length ``h`` that ends at ``t`` with the current u,
        formed and stored on the device (no synchronisation, no copy)."""
        self._check(self.lib.gmpnp_wall_profile_append(self._h, float(t), float(h)))

    def wall_profile_read(self, first, n) -> np.ndarray:
        """``gmpnp_wall_profile_read``: the records of steps ``first`` ... ``first + n - 1`` as a structured array (n, bins)
        (``WALL_PROFILE_RECORD_DTYPE``)."""
        return self._read_records(self.lib.gmpnp_wall_profile_read, WALL_PROFILE_RECORD_DTYPE, first, n, getattr(self, "_wall_profile_bins", 0))

    def wall_profile_close(self):
        """``gmpnp_wall_profile_close``."""
        self._check(self.lib.gmpnp_wall_profile_close(self._h))

    def sensitivity_open(self, params, start, capacity):
        """``gmpnp_sensitivity_open``: the state sensitivities S of the parameter codes ``params`` (``polarisation.PARAM_*``) and a
        record buffer of ``capacity`` steps.  ``start``: "zero" (S = 0), "steady" (S = the columns of a still-valid
        ``electrode_tangent`` call) or "continue" (S and the accumulators stay, the count is reset), or the C value 0 / 1 / 2."""
        pr = np.ascontiguousarray(params, dtype=np.int32).ravel()
        code = SENSITIVITY_START[start] if isinstance(start, str) else int(start)
        self._check(self.lib.gmpnp_sensitivity_open(self._h, int(pr.size), _iptr(pr), code, int(capacity)))
        self._n_sensitivities = int(pr.size)

    def sensitivity_step(self, t, h):
        """``gmpnp_sensitivity_step``: the recursion of the accepted step of length ``h`` that ends at ``t`` with the current u and the
        step's inv_dt, and one record per column, formed and stored on the device (no synchronisation, no copy)."""
        self._check(self.lib.gmpnp_sensitivity_step(self._h, float(t), float(h)))

    def sensitivity_read(self, first, n_steps) -> np.ndarray:
        """``gmpnp_sensitivity_read``: the records of steps ``first`` ... ``first + n_steps - 1`` as a structured array
        (``SENSITIVITY_RECORD_DTYPE``) of shape (n_steps, n columns)."""
        return self._read_records(self.lib.gmpnp_sensitivity_read, SENSITIVITY_RECORD_DTYPE, first, n_steps, getattr(self, "_n_sensitivities", 1))

    def sensitivity_columns(self, which=0) -> np.ndarray:
        """``gmpnp_sensitivity_columns``: S (``which`` = 0) or the right-hand sides of the last step (1), (n, ndof) in file order."""
        out = np.empty((getattr(self, "_n_sensitivities", 1), self.ndof))
        self._check(self.lib.gmpnp_sensitivity_columns(self._h, int(which), _dptr(out)))
        return out

    def sensitivity_set_columns(self, S):
        """``gmpnp_sensitivity_set_columns``: S <- ``S`` (n, ndof) in file order (the tests' hook)."""
        a = np.ascontiguousarray(S, dtype=np.float64)
        if a.shape != (getattr(self, "_n_sensitivities", 1), self.ndof):
            raise ValueError("sensitivities: S has the shape (n, ndof) of the open buffer")
        self._check(self.lib.gmpnp_sensitivity_set_columns(self._h, _dptr(a)))

    def sensitivity_close(self):
        """``gmpnp_sensitivity_close``."""
        self._check(self.lib.gmpnp_sensitivity_close(self._h))

    def set_supg(self, rho=None, w_index=None):
        """Nodal SUPG parameters (nv, ns) of the PNP stabilisation (reference 1D:597-722), or None to switch it off."""
        if rho is None:
            self._check(self.lib.gmpnp_set_supg(self._h, None, None))
            return
        rho = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
        assert rho.size == (self.ndof // self.nf) * (self.nf - 1)
        w = None if w_index is None else np.ascontiguousarray(w_index, dtype=np.int32)
        self._check(self.lib.gmpnp_set_supg(self._h, _dptr(rho), None if w is None else _iptr(w)))

    # ---- device-pointer variants: arguments are device addresses (e.g. ``torch.Tensor.data_ptr()`` of contiguous fp64
    # tensors of length ndof on this handle's GPU, file vertex order); the caller synchronises its own stream first ----
    def newton_solve(self, options: CNewtonOptions, error_on_nonconvergence=True):
        """``solve(F == 0, u, bcs, solver_parameters)`` on the device state.  Raises RuntimeError on
        non-convergence like [3P] DOLFIN (error_on_nonconvergence=True)."""
        st = CNewtonStats()
        code = self.lib.gmpnp_newton_solve(self._h, byref(options), byref(st))
        stats = dict(self.stats_dict(st), ms_assemble=st.ms_assemble, ms_setup=st.ms_setup, ms_krylov=st.ms_krylov)
        if code == ERR_NOT_CONVERGED and not error_on_nonconvergence:
            return stats
        if code != OK:
            raise GmpnpError(code, self.lib.gmpnp_last_error().decode(), stats=stats)
        return stats

    @staticmethod
    def stats_dict(st: "CNewtonStats"):
        return {"iterations": st.iterations, "converged": bool(st.converged), "krylov_iterations": st.krylov_iterations,
                "residuals": [st.residuals[i] for i in range(st.n_residuals)],
                "krylov_per_iteration": [st.krylov_per_iteration[i] for i in range(min(st.iterations, MAX_HISTORY))],
                "ms_total": st.ms_total, "direct_solves": st.direct_solves, "steric_excursion": st.steric_excursion,
                "limited_steps": st.limited_steps, "min_step": st.min_step,
                "step_factor": [st.step_factor[i] for i in range(min(st.iterations, MAX_HISTORY))]}

    def step_limit(self, dx, tau: float):
        """The step limiter's rule at the current u for the correction `dx` (file order), evaluated by the Newton loop's kernels
        (gmpnp_step_limit): (alpha, lambda, limiting vertex in file numbering or -1).  Changes nothing on the handle."""
        dx = np.ascontiguousarray(dx, dtype=np.float64).ravel()
        assert dx.size == self.ndof
        alpha, lam, node = c_double(), c_double(), c_int64()
        self._check(self.lib.gmpnp_step_limit(self._h, _dptr(dx), float(tau), byref(alpha), byref(lam), byref(node)))
        return alpha.value, lam.value, int(node.value)

    def set_time_step(self, inv_dt: float):
        """model.inv_dt alone, on this handle and every coarse level attached below it (gmpnp_set_time_step); 0 = steady form."""
        self._check(self.lib.gmpnp_set_time_step(self._h, float(inv_dt)))
        self.problem.model = dataclasses.replace(self.problem.model, inv_dt=float(inv_dt))   # what a later set_model re-uploads

    def time_error(self, h: float, h_prev: float, rtol: float, atol):
        """Backward Euler's local error and the rate of change of the step u_n -> u of length h (gmpnp_time_error; h_prev = the
        accepted step before it, <= 0: none).  ``atol``: a scalar or one value per field.  A dict with err, err_field, rate,
        rate_field (arrays of nf), worst_dof (file order, -1: none), has_history and nonfinite."""
        return time_error_call(self.lib.gmpnp_time_error, self._h, self.nf, self._check, h, h_prev, rtol, atol)

    def time_accept(self):
        """u_nm1 <- u_n, u_n <- u in one launch (gmpnp_time_accept): what an adaptive run calls instead of ``assign_previous``."""
        self._check(self.lib.gmpnp_time_accept(self._h))

    def time_reject(self):
        """u <- u_n (gmpnp_time_reject); the history stays."""
        self._check(self.lib.gmpnp_time_reject(self._h))

    # second order: variable-step BDF2 (include/gmpnp.h "second-order adaptive time stepping")
    def set_time_order(self, order: int):
        """1 = backward Euler (the default), 2 = variable-step BDF2 (gmpnp_set_time_order): 2 allocates u_nm2 and u*, and
        ``time_accept`` shifts three deep from then on."""
        self._check(self.lib.gmpnp_set_time_order(self._h, int(order)))

    def time_history_levels(self) -> int:
        """Accepted states behind u_n: 0, 1 (u_nm1) or 2 (u_nm1 and u_nm2) (gmpnp_time_history_levels)."""
        n = c_int32()
        self._check(self.lib.gmpnp_time_history_levels(self._h, byref(n)))
        return int(n.value)

    def set_time_step_bdf2(self, inv_dt: float, ratio: float):
        """The set-up of a BDF2 step of length h after an accepted step h_prev, ``ratio`` = h / h_prev (gmpnp_set_time_step_bdf2):
        model.inv_dt = alpha0 * ``inv_dt`` here and on the attached coarse levels, the time term reads u*."""
        self._check(self.lib.gmpnp_set_time_step_bdf2(self._h, float(inv_dt), float(ratio)))
        a0 = (1.0 + 2.0 * float(ratio)) / (1.0 + float(ratio))
        self.problem.model = dataclasses.replace(self.problem.model, inv_dt=a0 * float(inv_dt))

    def time_error_bdf2(self, h: float, h_prev: float, h_prev2: float, rtol: float, atol):
        """BDF2's local error of the step u_n -> u of length h (gmpnp_time_error_bdf2; h_prev, h_prev2: the two accepted steps
        before it).  The dict of ``time_error``; fewer than 2 levels: has_history False and err 0."""
        fn = lambda hd, a, b, tol, e: self.lib.gmpnp_time_error_bdf2(hd, a, b, float(h_prev2), tol, e)
        return time_error_call(fn, self._h, self.nf, self._check, h, h_prev, rtol, atol)

    def get_time_history(self):
        """u* of the last ``set_time_step_bdf2``, file order (gmpnp_get_time_history; for tests)."""
        out = np.empty(self.ndof)
        self._check(self.lib.gmpnp_get_time_history(self._h, _dptr(out)))
        return out

    def time_kernel(self, kernel: int, launches: int = 50) -> float:
        us = c_double()
        self._check(self.lib.gmpnp_time_kernel(self._h, kernel, launches, byref(us)))
        return us.value

    def event_overhead(self, pairs: int = 200) -> float:
        us = c_double()
        self._check(self.lib.gmpnp_event_overhead(self._h, pairs, byref(us)))
        return us.value

    def spmv_profile(self):
        n, mean, launched = c_int64(), c_double(), c_int64()
        self._check(self.lib.gmpnp_spmv_profile(self._h, byref(n), byref(mean), byref(launched)))
        return {"sampled": n.value, "mean_us": mean.value, "launched": launched.value}


def attach_level_chain(handles, parents, theta: float = 2.0, sweeps: int = 4):
    """The multilevel term over `handles` (finest first): handles[k + 1] attached below handles[k] with `parents[k]`, the table of
    level k's vertices in level k + 1, from the finest level to the coarsest (``DeviceSolver.attach_coarse_level``)."""
    for finer, coarse, par in zip(handles, handles[1:], parents):
        finer.attach_coarse_level(coarse, par, theta=theta, sweeps=sweeps)


MAX_ENSEMBLE = 64   # gmpnp_ensemble_create refuses more members


def column_select_call(fn, handle, fields, ranks, check):
    """One gmpnp_column_select / gmpnp_group_column_select call: (values, nan flag)."""
    f = np.ascontiguousarray(fields, dtype=np.int32).ravel()
    r = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
    if f.shape != r.shape:
        raise ValueError("fields and ranks differ in length")
    out = np.empty(f.size)
    flags = c_int32(0)
    check(fn(handle, f.size, _iptr(f), r.ctypes.data_as(POINTER(c_int64)), _dptr(out), byref(flags)))
    return out, bool(flags.value & 1)


def _fill_time_tol(tol, nf, rtol, atol):
    tol.rtol = float(rtol)
    a = np.broadcast_to(np.asarray(atol, dtype=np.float64), (nf,))
    for f in range(nf):
        tol.atol[f] = float(a[f])


def _time_error_dict(e, nf):
    return {"err": e.err, "err_field": np.array(e.err_field[:nf]), "rate": e.rate, "rate_field": np.array(e.rate_field[:nf]),
            "worst_dof": int(e.worst_dof), "has_history": bool(e.has_history), "nonfinite": bool(e.nonfinite)}


def time_error_call(fn, handle, nf, check, h, h_prev, rtol, atol):
    """One gmpnp_time_error call: the struct as a dict (per-field arrays cut to nf)."""
    tol = CTimeTol()
    _fill_time_tol(tol, nf, rtol, atol)
    e = CTimeError()
    check(fn(handle, float(h), float(h_prev), byref(tol), byref(e)))
    return _time_error_dict(e, nf)


def species_budget_call(fn, handle, nf, check):
    """One gmpnp_species_budget / gmpnp_group_species_budget call: the (nf, len(BUDGET_COLUMNS)) table."""
    out = np.empty((nf, len(BUDGET_COLUMNS)))
    check(fn(handle, _dptr(out)))
    return out


class DeviceEnsemble:
    """``gmpnp_ensemble``: the Newton solves of several ``DeviceSolver`` handles on ONE mesh in one launch chain per iteration
    (include/gmpnp.h): all of them 1D, or all of them 3D handles created with ``shared_device=1`` (solved with the two-level or the
    node-block Jacobi BiCGStab).  The members stay owned by the caller and keep their own surface (set_model, set_state, get_state,
    project_gradient, ...); every call here is complete when it returns."""

    def __init__(self, devices, lib=None):
        self.lib = lib or load_library()
        self.devices = list(devices)
        self._h = None
        arr = (c_void_p * max(1, len(self.devices)))(*[d._h for d in self.devices])
        h = c_void_p()
        self._check(self.lib.gmpnp_ensemble_create(len(self.devices), arr, byref(h)))
        self._h = h
        self.ndof = self.devices[0].ndof

    def _check(self, code):
        if code != OK:
            raise GmpnpError(code, self.lib.gmpnp_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gmpnp_ensemble_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return len(self.devices)

    def newton_solve(self, options: CNewtonOptions):
        """One Newton solve of every member.  Returns (stats, codes, messages): per member the statistics dict of
        ``DeviceSolver.newton_solve``, its gmpnp_status and the library's message of its failure ("" if none)."""
        n = len(self.devices)
        st = (CNewtonStats * n)()
        codes = (c_int32 * n)()
        rc = self.lib.gmpnp_ensemble_newton_solve(self._h, byref(options), st, codes)
        if rc != OK and not any(codes):   # refused before any member ran
            self._check(rc)
        stats = [DeviceSolver.stats_dict(st[k]) for k in range(n)]
        msgs = [self.lib.gmpnp_ensemble_member_error(self._h, k).decode() for k in range(n)]
        return stats, [int(c) for c in codes], msgs

    def assign_previous(self):
        self._check(self.lib.gmpnp_ensemble_assign_previous(self._h))

    def get_state(self):
        """u of every member, (n, n_dofs) in file order (one device-to-host copy)."""
        out = np.empty((len(self.devices), self.ndof))
        self._check(self.lib.gmpnp_ensemble_get_state(self._h, _dptr(out)))
        return out

    # adaptive time stepping, every member on its own clock (include/gmpnp.h; the round lives in timestep.EnsembleStepper)
    def set_time_step(self, inv_dts):
        """model.inv_dt of every member (gmpnp_ensemble_set_time_step): one value per member, one synchronisation for all."""
        x = np.ascontiguousarray(inv_dts, dtype=np.float64).ravel()
        if x.size != len(self.devices):
            raise ValueError("one inv_dt per member: %d values for %d members" % (x.size, len(self.devices)))
        self._check(self.lib.gmpnp_ensemble_set_time_step(self._h, _dptr(x)))

    def time_error(self, h, h_prev, rtol, atol, mask=None):
        """``DeviceSolver.time_error`` of every member with mask[k] true (None: all) in one launch chain
        (gmpnp_ensemble_time_error).  ``h``, ``h_prev``, ``rtol`` and ``atol`` hold one entry per member (``atol[k]`` a scalar or
        one value per field).  Returns the list of the members' dicts; a masked-out member's is all zero."""
        n, nf = len(self.devices), self.devices[0].nf
        hh = np.ascontiguousarray(h, dtype=np.float64).ravel()
        hp = np.ascontiguousarray(h_prev, dtype=np.float64).ravel()
        if not (hh.size == hp.size == len(rtol) == len(atol) == n) or (mask is not None and len(mask) != n):
            raise ValueError("h, h_prev, rtol, atol and mask hold one entry per member (%d)" % n)
        tol = (CTimeTol * n)()
        for k in range(n):
            _fill_time_tol(tol[k], nf, rtol[k], atol[k])
        m = None if mask is None else np.ascontiguousarray([1 if x else 0 for x in mask], dtype=np.int32)
        out = (CTimeError * n)()
        self._check(self.lib.gmpnp_ensemble_time_error(self._h, _dptr(hh), _dptr(hp), tol, None if m is None else _iptr(m), out))
        return [_time_error_dict(out[k], nf) for k in range(n)]

    def time_advance(self, actions):
        """Per member 0 = leave alone, 1 = ``time_accept``, 2 = ``time_reject``, in one launch (gmpnp_ensemble_time_advance)."""
        a = np.ascontiguousarray(actions, dtype=np.int32).ravel()
        if a.size != len(self.devices):
            raise ValueError("one action per member: %d values for %d members" % (a.size, len(self.devices)))
        self._check(self.lib.gmpnp_ensemble_time_advance(self._h, _iptr(a)))
