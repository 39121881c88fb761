"""ctypes binding of the C ABI (include/lscqp.h -> liblscqp.so).  Plumbing for tests and bench.py only.

The product is the shared library (HIP kernels + C ABI) and the C++ shim in lsc_dr_planner_amd/shim/.  This module
only moves bytes: numpy structured arrays for host calls, torch CUDA tensors (raw device pointers) for resident
calls.  It never computes anything and has NO CPU fallback: if liblscqp.so is missing, importing fails loudly.
"""
import ctypes as C
import math
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LSCQP_LIB") or os.path.join(_HERE, "liblscqp.so")  # (LSCQP_LIB: A/B builds of the development tools)

STATUS_OPTIMAL, STATUS_INFEASIBLE, STATUS_ITER_LIMIT, STATUS_NUMERIC, STATUS_CAPACITY = 0, 1, 2, 3, 4
PRECISION_F64, PRECISION_MIXED = 0, 1  # lscqp_class_desc.precision
WARM_DEFAULT, WARM_TIGHT = 0, 1  # lscqp_class_desc.warm_start
INFO_FLOOR_ACCEPTED, INFO_REPAIRED, INFO_RECENTRED, INFO_REMEMBERED, INFO_SHIFTED, INFO_RESCUED, INFO_ACTIVE_SET = 1, 2, 4, 8, 16, 32, 64  # lscqp_info.flags
INFO_PRESCREENED = 128  # lscqp_info.flags: INFEASIBLE by the prescreen (lscqp_set_prescreen)
PRESCREEN_OFF, PRESCREEN_ON = 0, 1  # lscqp_set_prescreen
ACTIVE_SET_DEFAULT, ACTIVE_SET_OFF, ACTIVE_SET_ONLY = 0, 1, 2  # lscqp_class_desc.active_set
(DAS_WHY_CAPACITY, DAS_WHY_EMPTY_INTERVAL, DAS_WHY_ROWS, DAS_WHY_STEPS, DAS_WHY_NO_STEP, DAS_WHY_PIVOT, DAS_WHY_VERIFICATION,
 DAS_WHY_MULTIPLIER) = range(1, 9)
PLANNER_DLSC, PLANNER_LSC, PLANNER_BVC, PLANNER_RSFC = 0, 1, 2, 3
OK, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_HIP = 0, 1, 2, 3, 4
SFC_INIT, SFC_FROM_HULL, SFC_FROM_POINT = 0, 1, 2  # lscqp_construct_sfc_device modes
GEN_LSC, GEN_CLSC, GEN_BVC = 0, 1, 2  # lscqp_generate_constraints_device modes (include/lscqp.h)

HEADER_DTYPE = np.dtype([
    ("p0", "f8", 3), ("v0", "f8", 3), ("a0", "f8", 3), ("goal", "f8", 3), ("next_waypoint", "f8", 3),
    ("vmax", "f8", 3), ("amax", "f8", 3), ("radius", "f8"), ("nominal_velocity", "f8"),
    ("n_obs", "i4"), ("terminal_segments", "i4"), ("reserved", "u4", 2), ("pad", "f8", 7),
])
ROW_DTYPE = np.dtype([("nx", "f8"), ("ny", "f8"), ("nz", "f8"), ("b", "f8")])
ROW_F32_DTYPE = np.dtype([("nx", "f4"), ("ny", "f4"), ("nz", "f4"), ("b", "f4")])  # lscqp_row_f32 (row_format = ROWS_F32)
ROWS_F64, ROWS_F32 = 0, 1
BOX_DTYPE = np.dtype([("bmin", "f8", 3), ("bmax", "f8", 3)])
SAFETY_DTYPE = np.dtype([("safety_ratio", "f8"), ("closest_agent", "i4"), ("sample", "i4"), ("vel_excess_ratio", "f8", 3),
                         ("acc_excess_ratio", "f8", 3)])
SAFETY_OBS_DTYPE = np.dtype([("safety_ratio_obs", "f8"), ("closest_obstacle", "i4"), ("sample", "i4")])  # lscqp_safety_obs
OBSTACLE_REAL = 2
OBSTACLE_DTYPE = np.dtype([("position", "f8", 3), ("velocity", "f8", 3), ("radius", "f8"), ("downwash", "f8"), ("max_acc", "f8"),
                           ("type", "i4"), ("reserved", "i4")])  # lscqp_obstacle
# lscqp_obstacle_model: how one dynamic obstacle moves (include/lscqp.h, "dynamic obstacles in the chain"); the fields from n_legs on are
# filled by obstacle_model_prepare
OBSTACLE_MAX_WAYPOINTS = 8
OBSTACLE_HELD, OBSTACLE_STRAIGHT, OBSTACLE_PATROL, OBSTACLE_SPIN = 0, 1, 2, 3  # lscqp_obstacle_model.kind
OBSTACLE_LEG_DTYPE = np.dtype([("start", "f4", 3), ("goal", "f4", 3), ("n", "f4", 3), ("reserved", "f4"), ("dist_to_goal", "f8"), ("dist_acc", "f8"),
                               ("flight_time", "f8")])
OBSTACLE_MODEL_DTYPE = np.dtype([("kind", "i4"), ("n_waypoints", "i4"), ("radius", "f8"), ("downwash", "f8"), ("max_acc", "f8"), ("speed", "f8"),
                                 ("start", "f8", 3), ("goal", "f8", 3), ("waypoints", "f8", (OBSTACLE_MAX_WAYPOINTS, 3)), ("axis_point", "f8", 3),
                                 ("axis_direction", "f8", 3), ("n_legs", "i4"), ("prepared", "i4"), ("leg", OBSTACLE_LEG_DTYPE, OBSTACLE_MAX_WAYPOINTS),
                                 ("lap_time", "f8"), ("spin_axis", "f8", 3), ("spin_offset", "f8", 3), ("spin_w", "f8")])
assert OBSTACLE_LEG_DTYPE.itemsize == 64 and OBSTACLE_MODEL_DTYPE.itemsize == 912
PLAN_OBS_TABLE, PLAN_OBS_SAFETY, PLAN_OBS_CLOCK = 0, 1, 2  # lscqp_plan_obstacle_buffer
# lscqp_obstacle_drive: how a chasing or gaussian obstacle is moved on the device (include/lscqp.h, "chasing and gaussian obstacles"), and
# lscqp_obstacle_drive_state, the gaussian obstacle's checkpoint
DRIVE_NONE, DRIVE_CHASING, DRIVE_GAUSSIAN = 0, 1, 2  # lscqp_obstacle_drive.kind
OBSTACLE_HISTORY_ENDED = 1                           # bit 0 of lscqp_obstacle.reserved
OBSTACLE_DRIVE_DTYPE = np.dtype([("kind", "i4"), ("target_agent", "i4"), ("max_vel", "f8"), ("gamma_target", "f8"), ("gamma_obs", "f8"), ("goal", "f8", 3),
                                 ("initial_vel", "f8", 3), ("acc_update_cycle", "f8"), ("history_first", "i4"), ("history_len", "i4")])
OBSTACLE_DRIVE_STATE_DTYPE = np.dtype([("i_done", "i4"), ("reserved", "i4"), ("position", "f4", 3), ("velocity", "f4", 3), ("v", "f8", 3)])
assert OBSTACLE_DRIVE_DTYPE.itemsize == 96 and OBSTACLE_DRIVE_STATE_DTYPE.itemsize == 56
# lscqp_plan_patrol_buffer (include/lscqp.h, "patrol missions")
(PATROL_DESIRED, PATROL_START, PATROL_LEGS, PATROL_SWAPPED, PATROL_FIELD, PATROL_INIT_D, PATROL_FIELD_OTHER, PATROL_INIT_D_OTHER) = range(8)
PATROL_COUNT = 8


class PatrolDesc(C.Structure):  # lscqp_patrol_desc
    _fields_ = [("goal_threshold", C.c_double)]


class ObstacleParam(C.Structure):  # lscqp_obstacle_param
    _fields_ = [("obs_uncertainty_horizon", C.c_double), ("velocity_guard_ratio", C.c_double), ("obs_downwash_threshold", C.c_double),
                ("reset_threshold", C.c_double), ("obs_size_prediction", C.c_int32), ("use_velocity_guard", C.c_int32)]


INFO_DTYPE = np.dtype([("iterations", "i4"), ("flags", "i4"), ("res_primal", "f8"), ("res_dual", "f8"),
                       ("gap", "f8")])
assert HEADER_DTYPE.itemsize == 256 and ROW_DTYPE.itemsize == 32 and BOX_DTYPE.itemsize == 48
assert INFO_DTYPE.itemsize == 32
# lscqp_diag (failure diagnostics): per row family the largest violation / count, and the most violated row by name
ROW_BOUND, ROW_SFC, ROW_LSC, ROW_VEL, ROW_ACC, ROW_COMM_PAIR, ROW_COMM_WAYPOINT, ROW_EQUALITY, ROW_FAMILIES = range(9)
PRESCREEN_CERT_DTYPE = np.dtype([("fired", "i4"), ("control_point", "i4"), ("n_rows", "i4"), ("reserved", "i4"), ("row", "i4", 4),
                                 ("lambda", "f8", 4), ("violation", "f8")])  # lscqp_prescreen_cert, 72 bytes
DIAG_DTYPE = np.dtype([("worst", "f8", 8), ("violated", "i4", 8), ("violation", "f8"), ("family", "i4"), ("obstacle", "i4"),
                       ("segment", "i4"), ("point", "i4"), ("axis", "i4"), ("reserved", "i4")])
assert DIAG_DTYPE.itemsize == 128


class ClassDesc(C.Structure):
    _fields_ = [
        ("M", C.c_int32), ("n", C.c_int32), ("phi", C.c_int32), ("phi_n", C.c_int32), ("dim", C.c_int32),
        ("planner_mode", C.c_int32), ("use_sfc", C.c_int32), ("row_format", C.c_int32),
        ("dt", C.c_double), ("control_input_weight", C.c_double), ("terminal_weight", C.c_double),
        ("communication_range", C.c_double), ("world_min", C.c_double * 3), ("world_max", C.c_double * 3),
        ("max_iter", C.c_int32), ("precision", C.c_int32), ("tol", C.c_double), ("warm_start", C.c_int32), ("active_set", C.c_int32),
    ]


class Work(C.Structure):  # lscqp_work
    _fields_ = [("flops_fixed", C.c_double), ("flops_per_iteration", C.c_double), ("flops_last_pass", C.c_double),
                ("f64_insts_per_iteration", C.c_double), ("valu_insts_per_iteration", C.c_double), ("lds_insts_per_iteration", C.c_double),
                ("valu_insts_fixed", C.c_double), ("wavefronts", C.c_int32), ("nslot", C.c_int32), ("max_obstacles", C.c_int32),
                ("lds_bytes", C.c_int32), ("kernel", C.c_char * 96)]


class _PlanPhase(C.Structure):  # csrc/lscqp_solve_plan.hpp: PhaseShape, Pass, SolvePlan -- what lscqp_debug_solve_plan_ fills
    _fields_ = [(k, C.c_int32) for k in ("cap", "threads", "kmax", "steps", "cacheC", "stage_rows", "screen", "tiny", "lds_bytes")]


class _PlanPass(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("kind", "repair", "scan", "queue", "x_init", "M", "dim", "es", "slots", "waves", "mixed")] + [
        ("inst", C.c_void_p), ("what", C.c_char_p)]


class _Plan(C.Structure):
    _fields_ = [("n_pass", C.c_int32), ("deferred", C.c_int32), ("error", C.c_int32), ("capacity", C.c_int32), ("phase", _PlanPhase),
                ("fused", C.c_void_p), ("passes", _PlanPass * 6)]


PLAN_WHOLE, PLAN_BEHIND_PHASE, PLAN_OTHER_ORDER, PLAN_RESCUE = 0, 1, 2, 3  # which part of a call (csrc/lscqp_solve_plan.hpp: SolvePart)
PLAN_PASS_KINDS = ("prescreen", "phase", "fused", "instance", "generic")    # PassKind
PLAN_ERRORS = (None, "lean_with_prescreen", "only_without_phase", "no_kernel")  # PlanError


class LscqpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lscqp error %d: %s" % (code, msg))
        self.code = code


_SCALARS = {"void": None, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
_STRUCTS = {"lscqp_class_desc": ClassDesc, "lscqp_work": Work, "SolvePlan": _Plan}  # the pointers that stay typed; every other one is void*


def _prototypes():
    """{name: (restype, argtypes)} of every `ret name(args);` of include/lscqp.h, and of the few library-internal entries that the wrappers
    below call for the tests.  The prototypes of liblscqp.so are written down once, in those two headers; this reads them from there."""
    texts = []
    for path in (os.path.join(_HERE, "..", "include", "lscqp.h"), os.path.join(_HERE, "csrc", "lscqp_internal.hpp")):
        if not os.path.exists(path):
            raise ImportError("cannot read the prototypes of liblscqp.so: %s is missing" % os.path.abspath(path))
        texts.append(re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(path).read(), flags=re.S))
    handles = set(re.findall(r"typedef\s+struct\s+\w+\s*\*\s*(\w+)\s*;", texts[0]))  # typedef struct lscqp_solver* lscqp_handle;

    def ctype(decl, named):
        words = re.sub(r"\b(const|struct)\b|\*", " ", decl).split()
        base, stars = words[0], decl.count("*")
        if "[" in decl or len(words) > 1 + named:
            raise ImportError("include/lscqp.h, csrc/lscqp_internal.hpp: cannot read the C type `%s`" % decl.strip())
        if stars == 0 and (base in _SCALARS or base in handles):
            return _SCALARS[base] if base in _SCALARS else C.c_void_p
        if stars == 1 and base == "char":
            return C.c_char_p
        if stars == 1 and base in _STRUCTS:
            return C.POINTER(_STRUCTS[base])
        if stars == 1 and base in handles:
            return C.POINTER(C.c_void_p)
        if stars:
            return C.c_void_p
        raise ImportError("include/lscqp.h, csrc/lscqp_internal.hpp: no ctypes type for the C type `%s`" % decl.strip())

    out = {}
    for text, names in zip(texts, (r"lscqp_\w+", r"lscqp_optimize_goal_fin_device_|lscqp_commit_validate_raw_|lscqp_debug_\w+_")):
        for ret, name, args in re.findall(r"^([\w ]+?[ *]+)(%s)\s*\(([^()]*)\)\s*;" % names, text, flags=re.M):
            args = [] if args.strip() in ("", "void") else args.split(",")
            out[name] = (ctype(ret, 0), [ctype(a, 1) for a in args])
    return out


_lib = None


def lib():
    """Load liblscqp.so.  Raises if it has not been built (python -m lsc_dr_planner_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("liblscqp.so not built: run `python lsc_dr_planner_amd/build.py` "
                              "(there is no CPU fallback)")
        # torch bundles its own libamdhip64 / libhsa-runtime64.  If liblscqp.so (linked against /opt/rocm's copy) is
        # loaded first, the process ends up with TWO HIP runtimes and the one that initialises second sees no device.
        # Importing torch first makes the loader resolve liblscqp.so's libamdhip64.so.7 to the copy torch already
        # loaded, so device pointers, streams and events are shared.  (The C++ shim has no torch and uses /opt/rocm.)
        import torch  # noqa: F401

        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _prototypes().items():
            if hasattr(L, name):  # (LSCQP_LIB may name an A/B build that predates an entry: tools/prescreen_timing.py, tools/solve_plan_ab.py)
                getattr(L, name).restype, getattr(L, name).argtypes = restype, argtypes
        _lib = L
    return _lib


def _arg(a):
    """One argument of an entry as ctypes takes it: a torch tensor is its device address, a numpy array its host address; None (a NULL
    pointer), numbers and ctypes values pass as they are."""
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a


def _call(name, *args, stream=False):
    """Call the entry `name` of liblscqp.so (its argtypes come from the headers, lib()) and raise LscqpError unless it returns OK.
    stream: for an entry whose last parameter is the stream -- a torch.cuda.Stream, or None for torch's current one; it is returned."""
    args = [_arg(a) for a in args]
    if stream is not False:
        if stream is None:
            import torch

            stream = torch.cuda.current_stream()
        args.append(C.c_void_p(stream.cuda_stream))
    rc = getattr(lib(), name)(*args)
    if rc != OK:
        raise LscqpError(rc, lib().lscqp_last_error().decode())
    return stream


def _stream_or_null(stream):
    """(an entry for which NULL means the default stream, passed among the arguments)"""
    return None if stream is None else C.c_void_p(stream.cuda_stream)


EXPORTED_SYMBOLS = ["lscqp_create", "lscqp_update", "lscqp_destroy", "lscqp_num_variables", "lscqp_num_inequalities",
                    "lscqp_algorithmic_bytes", "lscqp_solve_batch", "lscqp_solve_batch_stream", "lscqp_solve_batch_device", "lscqp_solve_batch_device_ex", "lscqp_solve_batch_device_ordered", "lscqp_order_by_work_device", "lscqp_launch_capacity", "lscqp_order_by_cost_device", "lscqp_construct_sfc_device_ordered",
                    "lscqp_num_segments", "lscqp_uses_sfc", "lscqp_row_bytes", "lscqp_max_obstacles", "lscqp_prepare_device", "lscqp_comm_prepare", "lscqp_comm_create", "lscqp_comm_destroy", "lscqp_comm_size",
                    "lscqp_comm_device", "lscqp_comm_stream", "lscqp_comm_backend", "lscqp_comm_set_min_agents_per_device",
                    "lscqp_comm_devices_for", "lscqp_comm_devices_for_class", "lscqp_device_fill", "lscqp_comm_shard", "lscqp_shard_range", "lscqp_exchange_schedule", "lscqp_exchange_schedule_padded", "lscqp_comm_synchronize", "lscqp_solve_batch_sharded",
                    "lscqp_solve_batch_sharded_device", "lscqp_allgather", "lscqp_generate_lsc_device", "lscqp_select_neighbours_device", "lscqp_generate_constraints_device",
                    "lscqp_shift_traj_device", "lscqp_shift_traj_partial_device", "lscqp_generate_constraints_device_ex",
                    "lscqp_generate_lsc_obstacles_device", "lscqp_generate_obstacle_rows_device", "lscqp_generate_lsc_bytes", "lscqp_optimize_goal_device", "lscqp_optimize_goal", "lscqp_validate_step_device", "lscqp_map_create", "lscqp_map_create_from_csv", "lscqp_map_destroy", "lscqp_map_info",
                    "lscqp_map_download", "lscqp_map_prepare", "lscqp_construct_sfc_device", "lscqp_construct_sfc", "lscqp_safety_metrics_device", "lscqp_safety_obstacles_device",
                    "lscqp_plan_create", "lscqp_plan_destroy", "lscqp_plan_reset", "lscqp_plan_buffer", "lscqp_plan_upload", "lscqp_plan_download",
                    "lscqp_plan_step", "lscqp_plan_step_graph", "lscqp_plan_graph_nodes", "lscqp_plan_group_step", "lscqp_plan_set_grid", "lscqp_plan_grid",
                    "lscqp_grid_shape", "lscqp_grid_create", "lscqp_grid_destroy", "lscqp_grid_info", "lscqp_grid_download", "lscqp_grid_download_mission",
                    "lscqp_grid_reserve", "lscqp_grid_status", "lscqp_grid_fields_device", "lscqp_waypoints_device",
                    "lscqp_grid_reserve_wide", "lscqp_waypoints_wide_device", "lscqp_plan_set_waypoint_decision",
                    "lscqp_plan_set_missions", "lscqp_plan_missions", "lscqp_plan_mission_status", "lscqp_select_neighbours_missions_device",
                    "lscqp_safety_metrics_missions_device", "lscqp_grid_fields_missions_device", "lscqp_waypoints_missions_device", "lscqp_grid_mission_status",
                    "lscqp_record_create", "lscqp_record_destroy", "lscqp_record_reset", "lscqp_record_step_device", "lscqp_record_download",
                    "lscqp_record_points", "lscqp_record_unfinished", "lscqp_plan_set_record", "lscqp_plan_record", "lscqp_plan_run",
                    "lscqp_record_set_log", "lscqp_record_log_obstacles", "lscqp_record_log", "lscqp_record_log_rows", "lscqp_record_log_download",
                    "lscqp_plan_set_flight_log",
                    "lscqp_record_set_obstacle_figures", "lscqp_record_obstacles_download", "lscqp_record_obstacles_raw", "lscqp_plan_set_obstacle_record",
                    "lscqp_obstacle_model_prepare", "lscqp_obstacles_advance_device", "lscqp_plan_set_obstacles", "lscqp_plan_obstacle_buffer",
                    "lscqp_plan_obstacle_upload", "lscqp_plan_obstacle_download",
                    "lscqp_obstacle_drive_check", "lscqp_obstacles_drive_device", "lscqp_obstacle_drive_host", "lscqp_plan_set_obstacle_drives",
                    "lscqp_obstacles_advance_missions_device", "lscqp_obstacles_drive_missions_device", "lscqp_safety_obstacles_ids_device",
                    "lscqp_plan_set_mission_obstacles",
                    "lscqp_patrol_check", "lscqp_patrol_device", "lscqp_patrol_host", "lscqp_field_exchange_device", "lscqp_plan_set_patrol",
                    "lscqp_plan_patrol_buffer",
                    "lscqp_worlds_create", "lscqp_worlds_destroy", "lscqp_worlds_prepare", "lscqp_worlds_info", "lscqp_construct_sfc_worlds_device",
                    "lscqp_grid_set_worlds", "lscqp_grid_download_world", "lscqp_plan_set_worlds",
                    "lscqp_instance_work", "lscqp_diagnose", "lscqp_diagnose_device", "lscqp_dump_instance", "lscqp_row_family_name",
                    "lscqp_prescreen_batch_device", "lscqp_set_prescreen", "lscqp_prescreen",
                    "lscqp_last_error", "lscqp_version"]


def make_desc(M=5, dim=3, dt=0.2, w_c=0.01, w_t=1.0, comm_range=3.0, planner_mode=PLANNER_LSC, use_sfc=True,
              world_min=(-5, -5, 0), world_max=(5, 5, 2.5), n=5, phi=3, phi_n=1, max_iter=0, tol=0.0, row_format=ROWS_F64,
              precision=PRECISION_F64, warm_start=0, active_set=0):
    d = ClassDesc()
    d.warm_start = warm_start
    d.active_set = active_set
    d.row_format = row_format
    d.precision = precision
    d.M, d.n, d.phi, d.phi_n, d.dim = M, n, phi, phi_n, dim
    d.planner_mode, d.use_sfc = planner_mode, int(use_sfc)
    d.dt, d.control_input_weight, d.terminal_weight, d.communication_range = dt, w_c, w_t, comm_range
    for k in range(3):
        d.world_min[k] = float(world_min[k])
        d.world_max[k] = float(world_max[k])
    d.max_iter, d.tol = max_iter, tol
    return d


def obstacle_models(specs):
    """OBSTACLE_MODEL_DTYPE records from a list of dicts in the reference's mission-file vocabulary (missions/*.json, "obstacles"):
    type ("straight", "patrol", "spin"; anything else -- "chasing", "gaussian", "real" -- is HELD at `start`), start, goal, waypoints, axis
    (a pose: position x y z and the axis direction in orientation x y z, or six numbers), size (the radius), speed, max_acc, downwash.
    Points are [x, y, z] or {"x":, "y":, "z":}.  Not prepared: obstacle_model_prepare or Plan.set_obstacles does that.  A chasing or gaussian
    entry moves on the device once it has a drive: obstacle_drives reads the same list, Plan.set_obstacle_drives takes the result."""
    def pt(v):
        return [float(v[k]) for k in ("x", "y", "z")] if isinstance(v, dict) else [float(c) for c in v]

    out = np.zeros(len(specs), OBSTACLE_MODEL_DTYPE)
    for m, o in zip(out, specs):
        kind = {"straight": OBSTACLE_STRAIGHT, "patrol": OBSTACLE_PATROL, "spin": OBSTACLE_SPIN}.get(o.get("type", "held"), OBSTACLE_HELD)
        m["kind"], m["radius"], m["downwash"] = kind, float(o.get("size", 0.15)), float(o.get("downwash", 1.0))
        m["max_acc"], m["speed"] = float(o.get("max_acc", 1.0)), float(o.get("speed", 0.0))
        if "start" in o:
            m["start"] = pt(o["start"])
        if "goal" in o:
            m["goal"] = pt(o["goal"])
        if kind == OBSTACLE_PATROL:
            wp = [pt(w) for w in o["waypoints"]]
            m["n_waypoints"] = len(wp)
            if len(wp) <= OBSTACLE_MAX_WAYPOINTS:  # (more: the library refuses the count)
                m["waypoints"][:len(wp)] = wp
                m["start"] = wp[0]
        if kind == OBSTACLE_SPIN:
            ax = o["axis"]
            if isinstance(ax, dict):
                pose = ax.get("pose", ax)
                m["axis_point"], m["axis_direction"] = pt(pose["position"]), pt(pose["orientation"])
            else:
                m["axis_point"], m["axis_direction"] = pt(ax[:3]), pt(ax[3:6])
    return out


def obstacle_model_prepare(models):
    """lscqp_obstacle_model_prepare on a copy of `models` (OBSTACLE_MODEL_DTYPE): checked, derived fields filled; no device needed."""
    m = np.array(models, dtype=OBSTACLE_MODEL_DTYPE, ndmin=1)
    _call("lscqp_obstacle_model_prepare", m, len(m))
    return m


def obstacle_drives(specs, n_total, horizon=60.0, seed=0):
    """(drives, acc_history) for the list obstacle_models takes: an OBSTACLE_DRIVE_DTYPE record per entry -- DRIVE_CHASING for "chasing",
    DRIVE_GAUSSIAN for "gaussian", DRIVE_NONE for everything else -- and the one shared [n_history][3] table of accelerations.  Field names are
    src/mission.cpp's (max_vel, gamma_target, gamma_obs; initial_vel, stddev_acc, acc_update_cycle, 0 = 0.1 s); optional keys: target_agent
    (a global agent id < n_total; default -1: fly to `goal`), goal (default the origin, what the reference's simulator passes), acc_history (a
    gaussian obstacle's own accelerations, [n][3]).  Without acc_history ceil(horizon / acc_update_cycle) accelerations are drawn from
    numpy.random.default_rng(seed), N(0, stddev_acc) per axis, and clamped to max_acc in norm (GaussianObstacle::update_acc_history)."""
    def pt(v):
        return [float(v[k]) for k in ("x", "y", "z")] if isinstance(v, dict) else [float(c) for c in v]

    rng = np.random.default_rng(seed)
    drives, hist = np.zeros(len(specs), OBSTACLE_DRIVE_DTYPE), []
    drives["target_agent"] = -1
    for d, o in zip(drives, specs):
        kind = o.get("type", "held")
        if kind == "chasing":
            d["kind"], d["max_vel"] = DRIVE_CHASING, float(o["max_vel"])
            d["gamma_target"], d["gamma_obs"] = float(o["gamma_target"]), float(o["gamma_obs"])
            d["target_agent"] = int(o.get("target_agent", -1))
            if not -1 <= d["target_agent"] < n_total:
                raise ValueError("target_agent %d outside [-1, %d)" % (d["target_agent"], n_total))
            d["goal"] = pt(o.get("goal", (0.0, 0.0, 0.0)))
        elif kind == "gaussian":
            d["kind"], d["max_vel"] = DRIVE_GAUSSIAN, float(o["max_vel"])
            d["initial_vel"] = pt(o.get("initial_vel", (0.0, 0.0, 0.0)))
            d["acc_update_cycle"] = float(o.get("acc_update_cycle", 0.0)) or 0.1
            if "acc_history" in o:
                acc = np.array(o["acc_history"], np.float64).reshape(-1, 3)
            else:
                max_acc = float(o.get("max_acc", 1.0))
                acc = rng.normal(0.0, float(o.get("stddev_acc", 0.0)), (int(math.ceil(horizon / d["acc_update_cycle"])), 3))
                norm = np.sqrt((acc * acc).sum(1))
                over = norm > max_acc
                acc[over] *= (max_acc / norm[over])[:, None]
            d["history_first"], d["history_len"] = sum(len(h) for h in hist), len(acc)
            hist.append(acc)
    return drives, (np.concatenate(hist) if hist else np.zeros((0, 3)))


def obstacle_drive_check(models, drives, n_history, n_total):
    """lscqp_obstacle_drive_check: raises LscqpError naming the model and the cause; no device needed."""
    m, d = np.ascontiguousarray(models, dtype=OBSTACLE_MODEL_DTYPE), np.ascontiguousarray(drives, dtype=OBSTACLE_DRIVE_DTYPE)
    if len(m) != len(d):
        raise ValueError("one drive per model")
    _call("lscqp_obstacle_drive_check", m, d, len(d), int(n_history), int(n_total))


def patrol_check(goal_threshold, n_agents, n_total):
    """lscqp_patrol_check: raises LscqpError naming the cause; no device needed."""
    _call("lscqp_patrol_check", C.byref(PatrolDesc(float(goal_threshold))), int(n_agents), int(n_total))


def pack_rows(lsc):
    """Reference LSC records (p, nrm, d) -> packed rows (nx, ny, nz, b = d + nrm.p); include/lscqp.h lscqp_row."""
    out = np.zeros(lsc.shape, ROW_DTYPE)
    out["nx"], out["ny"], out["nz"] = lsc["nrm"][..., 0], lsc["nrm"][..., 1], lsc["nrm"][..., 2]
    out["b"] = lsc["d"] + (lsc["nrm"] * lsc["p"]).sum(-1)
    return out


class WorldMap:
    """The voxel map of the corridor construction (lscqp_map): world boxes (n, 6) = centre xyz, size xyz -- the rows of the
    reference's world CSV -- or the CSV file itself; lives in HBM."""

    def __init__(self, boxes=None, world_min=(-5, -5, 0), world_max=(5, 5, 2.5), resolution=0.1, max_dist=1.0, csv_path=None):
        wmin = np.ascontiguousarray(world_min, dtype=np.float64)
        wmax = np.ascontiguousarray(world_max, dtype=np.float64)
        h = C.c_void_p()
        if csv_path is not None:
            _call("lscqp_map_create_from_csv", os.fsencode(csv_path), wmin, wmax, float(resolution), float(max_dist), C.byref(h))
        else:
            b = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
            _call("lscqp_map_create", b, b.shape[0], wmin, wmax, float(resolution), float(max_dist), C.byref(h))
        self._h = h
        dims, key0 = np.zeros(3, np.int32), np.zeros(3, np.int32)
        lib().lscqp_map_info(self._h, dims.ctypes.data_as(C.c_void_p), key0.ctypes.data_as(C.c_void_p))
        self.dims, self.key0 = dims, key0

    def prepare(self, max_radius):
        """lscqp_map_prepare: the free-space table that lets the corridor kernel pass tests in open space without sampling."""
        _call("lscqp_map_prepare", self._h, float(max_radius))

    def download(self):
        """(occ uint8, nearest int32), both shaped (dims[2], dims[1], dims[0])."""
        shape = (int(self.dims[2]), int(self.dims[1]), int(self.dims[0]))
        occ, near = np.zeros(shape, np.uint8), np.zeros(shape, np.int32)
        _call("lscqp_map_download", self._h, occ, near)
        return occ, near

    def close(self):
        if self._h:
            lib().lscqp_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Worlds:
    """lscqp_worlds: WorldMaps of one shape, world k for mission k (include/lscqp.h, "each mission over its own world").  The set borrows
    its maps: this object keeps them alive."""

    def __init__(self, maps):
        self._w = None
        self.maps = list(maps)
        arr = (C.c_void_p * max(len(self.maps), 1))(*[None if m is None else m._h for m in self.maps])
        h = C.c_void_p()
        _call("lscqp_worlds_create", arr, len(self.maps), C.byref(h))
        self._w = h

    def __len__(self):
        return len(self.maps)

    def prepare(self, max_radius):
        """lscqp_worlds_prepare: every member's free-space table with one margin."""
        _call("lscqp_worlds_prepare", self._w, float(max_radius))

    def info(self):
        """(n_worlds, dims int32[3], key0 int32[3]) of the common shape."""
        n, dims, key0 = C.c_int32(), np.zeros(3, np.int32), np.zeros(3, np.int32)
        _call("lscqp_worlds_info", self._w, C.byref(n), dims, key0)
        return int(n.value), dims, key0

    def close(self):
        if self._w:
            lib().lscqp_worlds_destroy(self._w)
            self._w = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GRID_UNREACHABLE = 0x3FFFFFFF  # LSCQP_GRID_UNREACHABLE


class GridDesc(C.Structure):  # lscqp_grid_desc
    _fields_ = [("resolution", C.c_double), ("radius", C.c_double), ("z_2d", C.c_double), ("world_dimension", C.c_int32), ("reserved_", C.c_int32)]


def grid_shape(world_min, world_max, resolution=0.5, world_dimension=2, z_2d=1.0):
    """lscqp_grid_shape (GridBasedPlanner::updateGridInfo): (grid_min float64[3], dims int32[3]).  No device call."""
    wmin, wmax = np.ascontiguousarray(world_min, dtype=np.float64), np.ascontiguousarray(world_max, dtype=np.float64)
    gmin, dims = np.zeros(3, np.float64), np.zeros(3, np.int32)
    _call("lscqp_grid_shape", wmin, wmax, float(resolution), int(world_dimension), float(z_2d), gmin, dims)
    return gmin, dims


def mission_offsets_arg(offsets, device=None, d_offsets=None):
    """A mission partition as the entry points take it: (K, host int64 array, its device copy or None).  offsets[0..K], see
    include/lscqp.h, "many missions over one map".  d_offsets: the caller's own device copy (an int64 tensor), kept by the caller."""
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if off.size < 2:
        raise ValueError("mission offsets: at least [0, n_total]")
    d_off = d_offsets
    if device is not None and d_off is None:
        import torch

        d_off = torch.from_numpy(off).to(device)
    return off.size - 1, off, d_off


class Grid:
    """lscqp_grid: the grid planner's grid over a WorldMap (include/lscqp.h, "the grid planner / MAPF layer"): occupancy, per-agent
    distance fields, and one replan's PIBT waypoint decision.  2-D.  `handle`: a grid owned by a Plan (not destroyed here)."""

    def __init__(self, world_map, resolution=0.5, radius=0.15, z_2d=1.0, world_dimension=2, handle=None):
        self._own = handle is None
        self._map = world_map
        if handle is None:
            d = GridDesc(float(resolution), float(radius), float(z_2d), int(world_dimension), 0)
            h = C.c_void_p()
            _call("lscqp_grid_create", world_map._h, C.byref(d), C.byref(h))
            handle = h
        self._h = handle
        self.grid_min, self.dims = np.zeros(3, np.float64), np.zeros(3, np.int32)
        lib().lscqp_grid_info(self._h, self.grid_min.ctypes.data_as(C.c_void_p), self.dims.ctypes.data_as(C.c_void_p))
        self.resolution = float(resolution)

    def close(self):
        if self._h and self._own:
            lib().lscqp_grid_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def download(self, mission=False):
        """Occupancy, uint8 (dims[1], dims[0]); mission=True: with the start and goal nodes of the last `fields` call cleared."""
        occ = np.zeros((int(self.dims[1]), int(self.dims[0])), np.uint8)
        _call("lscqp_grid_download_mission" if mission else "lscqp_grid_download", self._h, occ)
        return occ

    def set_worlds(self, worlds):
        """lscqp_grid_set_worlds: a base occupancy per world of a Worlds set (mission k starts from base k); None: the one base again."""
        _call("lscqp_grid_set_worlds", self._h, None if worlds is None else worlds._w)
        self._worlds = worlds

    def download_world(self, k):
        """lscqp_grid_download_world: the base occupancy of world k, uint8 (dims[1], dims[0])."""
        occ = np.zeros((int(self.dims[1]), int(self.dims[0])), np.uint8)
        _call("lscqp_grid_download_world", self._h, int(k), occ)
        return occ

    def status(self):
        st = np.zeros(1, np.int32)
        _call("lscqp_grid_status", self._h, st)
        return int(st[0])

    def reserve(self, n):
        _call("lscqp_grid_reserve", self._h, int(n))

    def fields(self, d_start_points, d_goal_points, d_field=None, d_init_d=None, stream=None):
        """lscqp_grid_fields_device: (d_field int32 (n, dims[1], dims[0]), d_init_d int32 (n,)), torch tensors on the device."""
        import torch

        n = d_start_points.numel() // 3
        if d_field is None:
            d_field = torch.empty((n, int(self.dims[1]), int(self.dims[0])), dtype=torch.int32, device=d_start_points.device)
        if d_init_d is None:
            d_init_d = torch.empty(n, dtype=torch.int32, device=d_start_points.device)
        _call("lscqp_grid_fields_device", self._h, n, d_start_points, d_goal_points, d_field, d_init_d, stream=stream)
        return d_field, d_init_d

    def waypoints(self, communication_range, M, dim, d_state, d_plan, d_current_goal, d_field, d_init_d, d_waypoint, stream=None):
        """lscqp_waypoints_device: d_waypoint (float64 (n, 3)) is updated in place; returns (group, desired node, updated), int32 (n,) tensors."""
        import torch

        n = d_waypoint.numel() // 3
        out = [torch.empty(n, dtype=torch.int32, device=d_waypoint.device) for _ in range(3)]
        _call("lscqp_waypoints_device", self._h, float(communication_range), int(M), int(dim), n, d_state, d_plan, d_current_goal, d_field, d_init_d,
              d_waypoint, *out, stream=stream)
        return tuple(out)

    def reserve_wide(self, n):
        """lscqp_grid_reserve_wide: the work arrays of `waypoints_wide` for n agents (those of `waypoints` included)."""
        _call("lscqp_grid_reserve_wide", self._h, int(n))

    def waypoints_wide(self, communication_range, M, dim, d_state, d_plan, d_current_goal, d_field, d_init_d, d_waypoint, stream=None):
        """lscqp_waypoints_wide_device: `waypoints` spread over the device; same arguments, the same outputs bit for bit."""
        import torch

        n = d_waypoint.numel() // 3
        out = [torch.empty(n, dtype=torch.int32, device=d_waypoint.device) for _ in range(3)]
        _call("lscqp_waypoints_wide_device", self._h, float(communication_range), int(M), int(dim), n, d_state, d_plan, d_current_goal, d_field, d_init_d,
              d_waypoint, *out, stream=stream)
        return tuple(out)

    def mission_status(self, n_missions):
        """lscqp_grid_mission_status: int32 (n_missions,), the word of each mission's waypoint walk."""
        st = np.zeros(int(n_missions), np.int32)
        _call("lscqp_grid_mission_status", self._h, int(n_missions), st)
        return st

    def fields_missions(self, offsets, d_start_points, d_goal_points, d_field=None, d_init_d=None, stream=None, d_offsets=None):
        """lscqp_grid_fields_missions_device: `fields` with one occupancy copy per mission of the partition `offsets` (host, [K + 1]).
        Without d_offsets (the caller's device copy of the offsets) the call makes its own and waits for the stream before it returns."""
        import torch

        n = d_start_points.numel() // 3
        K, off, d_off = mission_offsets_arg(offsets, d_start_points.device, d_offsets)
        if d_field is None:
            d_field = torch.empty((n, int(self.dims[1]), int(self.dims[0])), dtype=torch.int32, device=d_start_points.device)
        if d_init_d is None:
            d_init_d = torch.empty(n, dtype=torch.int32, device=d_start_points.device)
        s = _call("lscqp_grid_fields_missions_device", self._h, n, K, off, d_off, d_start_points, d_goal_points, d_field, d_init_d, stream=stream)
        if d_offsets is None:
            s.synchronize()  # (d_off is this call's own)
        return d_field, d_init_d

    def waypoints_missions(self, offsets, communication_range, M, dim, d_state, d_plan, d_current_goal, d_field, d_init_d, d_waypoint, stream=None,
                           d_offsets=None):
        """lscqp_waypoints_missions_device: `waypoints` as one decision per mission of the partition `offsets` (host, [K + 1]); d_offsets as
        for `fields_missions`."""
        import torch

        n = d_waypoint.numel() // 3
        K, off, d_off = mission_offsets_arg(offsets, d_waypoint.device, d_offsets)
        out = [torch.empty(n, dtype=torch.int32, device=d_waypoint.device) for _ in range(3)]
        s = _call("lscqp_waypoints_missions_device", self._h, float(communication_range), int(M), int(dim), n, K, off, d_off, d_state, d_plan,
                  d_current_goal, d_field, d_init_d, d_waypoint, *out, stream=stream)
        if d_offsets is None:
            s.synchronize()
        return tuple(out)


def waypoints(grid, communication_range, M, dim, d_state, d_plan, d_current_goal, d_field, d_init_d, d_waypoint, stream=None):
    """lscqp_waypoints_device (see Grid.waypoints)."""
    return grid.waypoints(communication_range, M, dim, d_state, d_plan, d_current_goal, d_field, d_init_d, d_waypoint, stream=stream)


# lscqp_mission_record (160 bytes)
MISSION_RECORD_DTYPE = np.dtype([("finished", "i4"), ("replans", "i4"), ("first_qp_failed_replan", "i4"), ("reserved", "i4"), ("flight_time", "f8"),
                                 ("distance", "f8"), ("safety_ratio_agent", "f8"), ("safety_replan", "i4"), ("safety_agent", "i4"), ("safety_other", "i4"),
                                 ("reserved2", "i4"), ("vel_excess_ratio", "f8", 3), ("acc_excess_ratio", "f8", 3), ("qp_failed", "i8"), ("invalid", "i8"),
                                 ("goal_failed", "i8"), ("sfc_kept", "i8"), ("waypoint_updates", "i8"), ("max_in_range", "i8"), ("truncated", "i8")])


# the obstacle record (include/lscqp.h, "the obstacle record"): lscqp_mission_obstacle_record (40 bytes), lscqp_agent_obstacle_record (24 bytes)
# and the spare bytes around the two arrays in the raw side buffer
MISSION_OBSTACLE_RECORD_DTYPE = np.dtype([("safety_ratio_obs", "f8"), ("replan", "i4"), ("agent", "i4"), ("obstacle", "i4"), ("sample", "i4"),
                                          ("below_one", "i8"), ("compared", "i8")])
AGENT_OBSTACLE_RECORD_DTYPE = np.dtype([("safety_ratio_obs", "f8"), ("replan", "i4"), ("obstacle", "i4"), ("sample", "i4"), ("reserved", "i4")])
OBSREC_SPARE = 64


# the flight log (include/lscqp.h, "the flight log"): the buffers of lscqp_record_log and the bits of a flags word
LOG_STATES, LOG_FLAGS, LOG_OBSTACLES = 0, 1, 2
LOG_FLAG_QP_FAILED, LOG_FLAG_INVALID, LOG_FLAG_GOAL_FAILED, LOG_FLAG_SFC_KEPT, LOG_FLAG_WAYPOINT = 1, 2, 4, 8, 16


class RecordDesc(C.Structure):  # lscqp_record_desc
    _fields_ = [("goal_threshold", C.c_double)]


class Record:
    """lscqp_record: per mission the running figures of the reference's summary line and the finish test, kept on the device
    (include/lscqp.h, "the mission record").  `handle`: a record owned by a Plan (not destroyed here)."""

    def __init__(self, solver=None, n_total=0, offsets=None, n_samples=2, record_time_step=0.1, time_step=0.2, z_2d=1.0, goal_threshold=0.1,
                 handle=None, n_missions=None):
        self._r, self._own = None, handle is None
        self.n_total, self.n_samples = int(n_total), int(n_samples)
        self.offsets = np.array([0, self.n_total], np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        self.log_capacity, self.log_n_dyn = 0, 0
        if handle is not None:
            self._r, self.n_missions = handle, int(n_missions)
            return
        d = RecordDesc(float(goal_threshold))
        K, off = 1, None
        if offsets is not None:
            K, off, _ = mission_offsets_arg(offsets)
        h = C.c_void_p()
        _call("lscqp_record_create", solver._h, self.n_total, K, off, self.n_samples, float(record_time_step), float(time_step), float(z_2d), C.byref(d),
              C.byref(h))
        self._r, self.n_missions, self._solver = h, K, solver

    def close(self):
        if self._r and self._own:
            lib().lscqp_record_destroy(self._r)
        self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, goal_points):
        gp = np.ascontiguousarray(goal_points, dtype=np.float64).reshape(self.n_total, 3)
        _call("lscqp_record_reset", self._r, gp)

    def step_device(self, d_hdr, d_x_all, d_status, d_goal_status, d_sfc_status, d_valid, d_in_range, d_safety, d_waypoint_updated=None, stream=None):
        _call("lscqp_record_step_device", self._r, d_hdr, d_x_all, d_status, d_goal_status, d_sfc_status, d_valid, d_in_range, d_safety, d_waypoint_updated,
              _stream_or_null(stream))

    def download(self):
        """(records (K,) MISSION_RECORD_DTYPE, agent distances (n_total,) float64); waits for the device."""
        rec = np.zeros(self.n_missions, MISSION_RECORD_DTYPE)
        dist = np.zeros(self.n_total, np.float64)
        _call("lscqp_record_download", self._r, rec, dist)
        return rec, dist

    def points(self):
        """The sample points of the last step, float32 (n_total, n_samples, 3), copied to the host (waits for the device)."""
        import torch

        nb = C.c_uint64()
        ptr = lib().lscqp_record_points(self._r, C.byref(nb))

        class _View:
            __cuda_array_interface__ = dict(shape=(nb.value // 4,), typestr="<f4", data=(ptr, False), version=2)

        torch.cuda.synchronize()
        return torch.as_tensor(_View(), device="cuda").cpu().numpy().reshape(self.n_total, self.n_samples, 3)

    def unfinished(self):
        w = C.c_int32()
        _call("lscqp_record_unfinished", self._r, C.byref(w))
        return int(w.value)

    def set_log(self, max_replans, n_dyn=0):
        """lscqp_record_set_log: a flight log of max_replans rows per mission with n_dyn obstacle columns (0 rows: none); waits for the device."""
        _call("lscqp_record_set_log", self._r, int(max_replans), int(n_dyn))
        self.log_capacity, self.log_n_dyn = int(max_replans), int(n_dyn) if max_replans else 0

    def log_obstacles(self, d_table):
        """lscqp_record_log_obstacles: the device table (OBSTACLE_DTYPE records, borrowed) the obstacle columns are read from; None: none."""
        _call("lscqp_record_log_obstacles", self._r, d_table)

    def log_tensor(self, which):
        """One raw buffer of the log (LOG_STATES / LOG_OBSTACLES float32, LOG_FLAGS int32) as a flat torch tensor over the device memory
        itself; the layout is include/lscqp.h's.  None for an empty buffer."""
        import torch

        nb = C.c_uint64()
        ptr = lib().lscqp_record_log(self._r, int(which), C.byref(nb))
        if not ptr:
            raise LscqpError(ERR_INVALID_ARGUMENT, lib().lscqp_last_error().decode())
        if nb.value == 0:
            return None

        class _View:
            __cuda_array_interface__ = dict(shape=(nb.value // 4,), typestr="<i4" if which == LOG_FLAGS else "<f4", data=(ptr, False), version=2)

        return torch.as_tensor(_View(), device="cuda")

    def log_rows(self):
        """lscqp_record_log_rows: (rows (K,) int32 = min(replans, capacity), overflowed (K,) int32); waits for the device."""
        rows, over = np.zeros(self.n_missions, np.int32), np.zeros(self.n_missions, np.int32)
        _call("lscqp_record_log_rows", self._r, rows, over)
        return rows, over

    def log(self, mission, first_replan=0, n_replans=None):
        """lscqp_record_log_download: one mission's rows [first_replan, first_replan + n_replans) -- all of them by default -- as
        (states (rows, n_k, S, 9) float32, flags (rows, n_k) int32, obstacles (rows, n_dyn, 4) float32); waits for the device."""
        k = int(mission)
        known = 0 <= k < self.n_missions  # (an unknown mission is the library's to refuse)
        if n_replans is None:
            n_replans = int(self.log_rows()[0][k]) - int(first_replan) if known else 0
        n, n_k = int(n_replans), int(self.offsets[k + 1] - self.offsets[k]) if known else 0
        st = np.zeros((max(n, 0), n_k, self.n_samples, 9), np.float32)
        fl = np.zeros((max(n, 0), n_k), np.int32)
        ob = np.zeros((max(n, 0), self.log_n_dyn, 4), np.float32)
        _call("lscqp_record_log_download", self._r, k, int(first_replan), n, st, fl, ob)
        return st, fl, ob


    def set_obstacle_figures(self, d_safety_obs):
        """lscqp_record_set_obstacle_figures: the device array (SAFETY_OBS_DTYPE records, n_total, borrowed) whose minimum the record keeps
        per mission and per agent from the next step on; None removes the obstacle record.  Waits for the device."""
        _call("lscqp_record_set_obstacle_figures", self._r, d_safety_obs)

    def obstacles(self):
        """lscqp_record_obstacles_download: (missions (K,) MISSION_OBSTACLE_RECORD_DTYPE, agents (n_total,) AGENT_OBSTACLE_RECORD_DTYPE);
        waits for the device."""
        ms = np.zeros(self.n_missions, MISSION_OBSTACLE_RECORD_DTYPE)
        ag = np.zeros(self.n_total, AGENT_OBSTACLE_RECORD_DTYPE)
        _call("lscqp_record_obstacles_download", self._r, ms, ag)
        return ms, ag

    def obstacles_tensor(self):
        """The obstacle record's raw side buffer as a flat uint8 torch tensor over the device memory itself: OBSREC_SPARE bytes, the missions'
        structs, OBSREC_SPARE bytes, the agents' structs, OBSREC_SPARE bytes (include/lscqp.h: lscqp_record_obstacles_raw)."""
        import torch

        nb = C.c_uint64()
        ptr = lib().lscqp_record_obstacles_raw(self._r, C.byref(nb))
        if not ptr:
            raise LscqpError(ERR_INVALID_ARGUMENT, lib().lscqp_last_error().decode())

        class _View:
            __cuda_array_interface__ = dict(shape=(nb.value,), typestr="|u1", data=(ptr, False), version=2)

        return torch.as_tensor(_View(), device="cuda")


AGENT_PARAM_DTYPE = np.dtype([("radius", "f8"), ("downwash", "f8"), ("max_vel", "f8", 3), ("max_acc", "f8", 3), ("nominal_velocity", "f8")])


class PlanDesc(C.Structure):  # lscqp_plan_desc
    _fields_ = [("n_agents", C.c_int64), ("n_total", C.c_int64), ("first_agent", C.c_int64), ("n_obs", C.c_int32), ("constraint_mode", C.c_int32),
                ("sfc_mode", C.c_int32), ("optimize_goal", C.c_int32), ("closed_loop", C.c_int32), ("safety_samples", C.c_int32),
                ("time_step", C.c_double), ("z_2d", C.c_double), ("record_time_step", C.c_double), ("tight_warm_start", C.c_int32),
                ("prediction_mode", C.c_int32), ("initial_traj_mode", C.c_int32), ("waypoint_mode", C.c_int32), ("reset_threshold", C.c_double)]


TRAJ_FROM_PREVIOUS_SOLUTION, TRAJ_FROM_POSITION, TRAJ_FROM_VELOCITY = 0, 1, 2
WAYPOINT_FROM_CALLER, WAYPOINT_GRID_PIBT = 0, 1
DECISION_ONE_WORKGROUP, DECISION_WIDE, DECISION_AUTO = 0, 1, 2
DECISION_AUTO_MIN_AGENTS = 512  # LSCQP_DECISION_AUTO_MIN_AGENTS


(PLAN_STATE, PLAN_WAYPOINT, PLAN_PLAN, PLAN_GOAL, PLAN_HEADER, PLAN_ROWS, PLAN_SFC, PLAN_STATUS, PLAN_GOAL_STATUS, PLAN_SFC_STATUS, PLAN_VALID,
 PLAN_IN_RANGE, PLAN_NEXT_STATE, PLAN_OBJECTIVE, PLAN_INFO, PLAN_SAFETY, PLAN_DESIRED_GOAL, PLAN_WAYPOINT_UPDATED, PLAN_GROUP) = range(19)


class Plan:
    """lscqp_plan: one replan of a batch of agents as one chain of device work (include/lscqp.h, "the caller of the path"), eager
    (`step`) or through a captured hipGraph (`step_graph`).  Buffers are addressed by the PLAN_* constants; `get` / `put` copy
    synchronously, `pointer` returns the device address."""

    _DT = {PLAN_STATE: np.float64, PLAN_WAYPOINT: np.float64, PLAN_PLAN: np.float64, PLAN_GOAL: np.float64, PLAN_STATUS: np.int32,
           PLAN_GOAL_STATUS: np.int32, PLAN_SFC_STATUS: np.int32, PLAN_VALID: np.int32, PLAN_IN_RANGE: np.int32, PLAN_NEXT_STATE: np.float64,
           PLAN_OBJECTIVE: np.float64, PLAN_DESIRED_GOAL: np.float64, PLAN_WAYPOINT_UPDATED: np.int32, PLAN_GROUP: np.int32}

    def __init__(self, solver, world_map, n_agents, n_obs, agents, n_total=None, first_agent=0, constraint_mode=1, sfc_mode=1,
                 optimize_goal=True, closed_loop=False, time_step=None, z_2d=1.0, safety_samples=0, record_time_step=0.1, tight_warm_start=False,
                 prediction_mode=TRAJ_FROM_PREVIOUS_SOLUTION, initial_traj_mode=TRAJ_FROM_PREVIOUS_SOLUTION, reset_threshold=0.1,
                 waypoint_mode=WAYPOINT_FROM_CALLER, grid_resolution=0.5, mission_offsets=None):
        self._p = None
        n_total = n_agents if n_total is None else n_total
        d = PlanDesc()
        d.n_agents, d.n_total, d.first_agent, d.n_obs = n_agents, n_total, first_agent, n_obs
        d.constraint_mode, d.sfc_mode, d.optimize_goal, d.closed_loop = constraint_mode, sfc_mode, int(optimize_goal), int(closed_loop)
        d.time_step = float(solver.desc.dt if time_step is None else time_step)
        d.z_2d = float(z_2d)
        d.safety_samples, d.record_time_step = int(safety_samples), float(record_time_step)
        d.tight_warm_start = int(tight_warm_start)
        d.prediction_mode, d.initial_traj_mode, d.reset_threshold = int(prediction_mode), int(initial_traj_mode), float(reset_threshold)
        d.waypoint_mode = int(waypoint_mode)
        ag = np.ascontiguousarray(agents, dtype=AGENT_PARAM_DTYPE)
        if ag.shape != (n_total,):
            raise ValueError("agents: one AGENT_PARAM_DTYPE record per agent of the mission")
        h = C.c_void_p()
        _call("lscqp_plan_create", solver._h, world_map._h if world_map is not None else None, C.byref(d), ag, C.byref(h))
        self._p, self._solver, self._map = h, solver, world_map  # (keeps the solver and the map alive)
        self.n_agents, self.n_total, self.first_agent, self.n_obs, self.M, self.nv = n_agents, n_total, first_agent, n_obs, solver.desc.M, solver.nv
        self.n_dyn = 0  # dynamic obstacles (set_obstacles)
        self._dt = dict(self._DT)
        self._dt.update({PLAN_HEADER: HEADER_DTYPE, PLAN_ROWS: ROW_DTYPE, PLAN_SFC: BOX_DTYPE, PLAN_INFO: INFO_DTYPE, PLAN_SAFETY: SAFETY_DTYPE})
        self.waypoint_mode, self.grid_resolution, self._safety_samples = int(waypoint_mode), float(grid_resolution), int(safety_samples)
        if self.waypoint_mode == WAYPOINT_GRID_PIBT and float(grid_resolution) != 0.5:
            _call("lscqp_plan_set_grid", self._p, float(grid_resolution))
        if mission_offsets is not None:
            try:
                self.set_missions(mission_offsets)
            except Exception:
                self.close()  # (a refused partition: the native plan does not wait for __del__)
                raise

    def set_missions(self, offsets):
        """lscqp_plan_set_missions: offsets[0..K] cut the agents into K independent missions over the plan's map (None or K <= 1: one
        mission).  Call it before `reset`."""
        K, off = (0, None) if offsets is None else mission_offsets_arg(offsets)[:2]
        _call("lscqp_plan_set_missions", self._p, K, off)

    def set_worlds(self, worlds):
        """lscqp_plan_set_worlds: world k of a Worlds set for mission k of the partition (None: the plan's one map again).  Call it after
        `set_missions` and before `reset`."""
        _call("lscqp_plan_set_worlds", self._p, None if worlds is None else worlds._w)
        self._worlds = worlds  # (the set, and through it its maps, stay alive with the plan)

    def set_waypoint_decision(self, which):
        """lscqp_plan_set_waypoint_decision: DECISION_ONE_WORKGROUP (default), DECISION_WIDE or DECISION_AUTO; waypoint_mode 1 only."""
        _call("lscqp_plan_set_waypoint_decision", self._p, int(which))

    def missions(self):
        """lscqp_plan_missions: the partition's offsets, int64 (K + 1,); [0, n_total] without one."""
        K = C.c_int32()
        _call("lscqp_plan_missions", self._p, C.byref(K), None)
        off = np.zeros(K.value + 1, np.int64)
        _call("lscqp_plan_missions", self._p, C.byref(K), off)
        return off

    def mission_status(self):
        """lscqp_plan_mission_status: int32 (K,), 1 where a mission's waypoint walk reached its bound."""
        st = np.zeros(len(self.missions()) - 1, np.int32)
        _call("lscqp_plan_mission_status", self._p, st)
        return st

    def grid(self):
        """The plan's own Grid (waypoint_mode = WAYPOINT_GRID_PIBT), for inspection; owned by the plan."""
        h = lib().lscqp_plan_grid(self._p)
        return None if not h else Grid(self._map, resolution=self.grid_resolution, handle=C.c_void_p(h))

    def close(self):
        if self._p:
            lib().lscqp_plan_destroy(self._p)
            self._p = None
        self._worlds = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, start_positions, goal_points=None):
        sp = np.ascontiguousarray(start_positions, dtype=np.float64).reshape(self.n_total, 3)
        gp = None if goal_points is None else np.ascontiguousarray(goal_points, dtype=np.float64).reshape(self.n_total, 3)
        _call("lscqp_plan_reset", self._p, sp, gp)

    def pointer(self, which):
        nb = C.c_uint64()
        ptr = lib().lscqp_plan_buffer(self._p, which, C.byref(nb))
        return ptr, nb.value

    def get(self, which):
        _, nb = self.pointer(which)
        out = np.zeros(nb // np.dtype(self._dt[which]).itemsize, dtype=self._dt[which])
        _call("lscqp_plan_download", self._p, which, out, 0, nb)
        return out

    def put(self, which, array, first=0):
        """array: entries [first, first + len) of the buffer, in units of the buffer's record (an agent's 9 doubles, ...)."""
        a = np.ascontiguousarray(array, dtype=self._dt[which])
        _, nb = self.pointer(which)
        per = {PLAN_STATE: 72, PLAN_WAYPOINT: 24, PLAN_GOAL: 24, PLAN_PLAN: 8 * self.nv, PLAN_SFC: 48 * self.M}.get(which)
        if per is None:
            raise ValueError("not an input buffer")
        _call("lscqp_plan_upload", self._p, which, a, first * per, a.nbytes)

    def tensor(self, which):
        """Zero-copy torch view of a float64 buffer of the plan (PLAN_PLAN, PLAN_STATE, PLAN_GOAL, ...): what
        sharding.exchange_plan_buffers exchanges between the ranks of a torch.distributed job."""
        import torch

        if np.dtype(self._dt[which]) != np.float64:
            raise ValueError("not a float64 buffer")
        ptr, nb = self.pointer(which)

        class _View:
            __cuda_array_interface__ = dict(shape=(nb // 8,), typestr="<f8", data=(ptr, False), version=2)

        return torch.as_tensor(_View(), device="cuda")

    def step(self, stream=None, graph=False):
        if getattr(self, "_solver", None) is not None:
            self._solver._sync_knobs()
        _call("lscqp_plan_step_graph" if graph else "lscqp_plan_step", self._p, _stream_or_null(stream))

    def graph_nodes(self):
        return int(lib().lscqp_plan_graph_nodes(self._p))

    def set_obstacles(self, models, param=None):
        """lscqp_plan_set_obstacles: models is an OBSTACLE_MODEL_DTYPE array (obstacle_models builds one from mission-file entries) or None /
        empty to take the obstacles away; param an ObstacleParam (default: the reference's launch-file values).  `reset` must follow."""
        if models is None or len(models) == 0:
            _call("lscqp_plan_set_obstacles", self._p, None, 0, None)
            self.n_dyn = 0
            return
        m = np.ascontiguousarray(models, dtype=OBSTACLE_MODEL_DTYPE)
        if param is None:
            param = ObstacleParam(1.0, 0.75, 3.0, 0.1, 1, 1)
        _call("lscqp_plan_set_obstacles", self._p, C.byref(param), len(m), m)
        self.n_dyn = len(m)

    def set_mission_obstacles(self, models_per_mission, param=None):
        """lscqp_plan_set_mission_obstacles: one OBSTACLE_MODEL_DTYPE array per mission of the partition in force (an empty one or None for a
        mission without obstacles), each mission's own -- its agents see no other's.  None, or no obstacle in any mission, takes the obstacles
        away; param as in set_obstacles.  `reset` must follow.  The table, the drives and PLAN_OBS_TABLE are mission-major; PLAN_OBS_CLOCK has
        one word per mission."""
        per = [] if models_per_mission is None else [np.zeros(0, OBSTACLE_MODEL_DTYPE) if m is None else np.ascontiguousarray(m, dtype=OBSTACLE_MODEL_DTYPE).reshape(-1)
                                                     for m in models_per_mission]
        off = np.zeros(len(per) + 1, np.int32)
        off[1:] = np.cumsum([len(m) for m in per])
        if off[-1] == 0:
            _call("lscqp_plan_set_mission_obstacles", self._p, None, 0, None, None)
            self.n_dyn = 0
            return
        m = np.ascontiguousarray(np.concatenate(per))
        if param is None:
            param = ObstacleParam(1.0, 0.75, 3.0, 0.1, 1, 1)
        _call("lscqp_plan_set_mission_obstacles", self._p, C.byref(param), len(per), off, m)
        self.n_dyn = len(m)

    def set_obstacle_drives(self, drives, acc_history=None):
        """lscqp_plan_set_obstacle_drives: an OBSTACLE_DRIVE_DTYPE record per obstacle of the plan and the shared [n_history][3] table of
        accelerations (obstacle_drives builds both), or None / empty to take the drives away.  `reset` must follow."""
        if drives is None or len(drives) == 0:
            _call("lscqp_plan_set_obstacle_drives", self._p, None, 0, None, 0)
            return
        d = np.ascontiguousarray(drives, dtype=OBSTACLE_DRIVE_DTYPE)
        h = np.ascontiguousarray(np.zeros((0, 3)) if acc_history is None else acc_history, dtype=np.float64).reshape(-1, 3)
        _call("lscqp_plan_set_obstacle_drives", self._p, d, len(d), h if len(h) else None, len(h))

    _OBS_DT ={PLAN_OBS_TABLE: OBSTACLE_DTYPE, PLAN_OBS_SAFETY: SAFETY_OBS_DTYPE, PLAN_OBS_CLOCK: np.int32}

    def obstacle_pointer(self, which):
        nb = C.c_uint64()
        ptr = lib().lscqp_plan_obstacle_buffer(self._p, which, C.byref(nb))
        return ptr, nb.value

    def get_obstacles(self, which=PLAN_OBS_TABLE):
        """The plan's obstacle table as the last replan's advance left it (OBSTACLE_DTYPE), or with which = PLAN_OBS_SAFETY / PLAN_OBS_CLOCK the
        obstacle safety figures / the clock; an empty array without obstacles."""
        _, nb = self.obstacle_pointer(which)
        out = np.zeros(nb // np.dtype(self._OBS_DT[which]).itemsize, dtype=self._OBS_DT[which])
        if nb:
            _call("lscqp_plan_obstacle_download", self._p, which, out, 0, nb)
        return out

    def put_obstacles(self, table, first=0):
        """Entries [first, first + len) of the table: the caller's to write for OBSTACLE_HELD models, between eager replans."""
        a = np.ascontiguousarray(table, dtype=OBSTACLE_DTYPE)
        _call("lscqp_plan_obstacle_upload", self._p, PLAN_OBS_TABLE, a, first * OBSTACLE_DTYPE.itemsize, a.nbytes)

    def set_patrol(self, goal_threshold=0.1):
        """lscqp_plan_set_patrol: the plan flies a patrol -- every agent swaps start and goal on arrival within goal_threshold (None: no
        patrol).  `reset` (with the goal points) must follow."""
        _call("lscqp_plan_set_patrol", self._p, None if goal_threshold is None else C.byref(PatrolDesc(float(goal_threshold))))

    _PATROL_DT = {PATROL_DESIRED: np.float64, PATROL_START: np.float64}  # (every other one: int32)

    def patrol_pointer(self, which):
        nb = C.c_uint64()
        ptr = lib().lscqp_plan_patrol_buffer(self._p, int(which), C.byref(nb))
        return ptr, nb.value

    def patrol(self, which):
        """lscqp_plan_patrol_buffer, downloaded (waits for the device): PATROL_DESIRED / PATROL_START (n_total, 3) float64, PATROL_LEGS /
        PATROL_SWAPPED / PATROL_INIT_D[_OTHER] (n_total,) int32, PATROL_FIELD[_OTHER] (n_total, nodes) int32; an empty array where the plan
        has none (no patrol, or a field entry without a grid)."""
        import torch

        ptr, nb = self.patrol_pointer(which)
        dt = np.dtype(self._PATROL_DT.get(which, np.int32))
        if not ptr or nb == 0:
            return np.zeros(0, dt)

        class _View:
            __cuda_array_interface__ = dict(shape=(nb // dt.itemsize,), typestr=dt.str, data=(ptr, False), version=2)

        torch.cuda.synchronize()
        out = torch.as_tensor(_View(), device="cuda").cpu().numpy()
        return out.reshape(self.n_total, -1) if which in (PATROL_DESIRED, PATROL_START, PATROL_FIELD, PATROL_FIELD_OTHER) else out

    def set_record(self, goal_threshold=0.1):
        """lscqp_plan_set_record: the plan keeps a mission record, accumulated by the chain's last node (None: no record).  `reset` must follow."""
        _call("lscqp_plan_set_record", self._p, None if goal_threshold is None else C.byref(RecordDesc(float(goal_threshold))))
        if goal_threshold is None:
            self._log_capacity = 0  # (the log goes with the record)

    def record(self):
        """The plan's own Record (owned by the plan), None without one."""
        h = lib().lscqp_plan_record(self._p)
        if not h:
            return None
        off = self.missions()
        rec = Record(handle=C.c_void_p(h), n_total=self.n_total, n_samples=self._safety_samples, n_missions=len(off) - 1, offsets=off)
        rec.log_capacity = getattr(self, "_log_capacity", 0)
        rec.log_n_dyn = int(getattr(self, "n_dyn", 0)) if rec.log_capacity else 0
        return rec

    def set_flight_log(self, max_replans):
        """lscqp_plan_set_flight_log: the plan's record keeps a flight log of max_replans rows per mission, with the plan's obstacle columns
        (0: none).  Needs `set_record` first; `reset` must follow."""
        _call("lscqp_plan_set_flight_log", self._p, int(max_replans))
        self._log_capacity = int(max_replans)

    def set_obstacle_record(self, on=True):
        """lscqp_plan_set_obstacle_record: the plan's record keeps each mission's least obstacle safety ratio over the flight, read with
        `record().obstacles()`.  Needs `set_record` and `set_obstacles` first; `reset` must follow."""
        _call("lscqp_plan_set_obstacle_record", self._p, int(bool(on)))

    def run(self, max_replans, check_every=1, graph=True, stream=None):
        """lscqp_plan_run: replans until every mission of the record has finished or max_replans; returns the replans enqueued."""
        if getattr(self, "_solver", None) is not None:
            self._solver._sync_knobs()
        n = C.c_int64()
        _call("lscqp_plan_run", self._p, int(max_replans), int(check_every), int(bool(graph)), _stream_or_null(stream), C.byref(n))
        return int(n.value)


def shard_range(n, n_used, g):
    """lscqp_shard_range: block [first, first + count) of device g when n agents are spread over n_used devices."""
    f, c = C.c_int64(), C.c_int64()
    _call("lscqp_shard_range", n, n_used, g, C.byref(f), C.byref(c))
    return f.value, c.value


XCHG_ALLGATHER, XCHG_BROADCAST = 0, 1
EXCHANGE_OP_DTYPE = np.dtype([("kind", "<i4"), ("root", "<i4"), ("offset", "<i8"), ("count", "<i8")])


PLAN_EXCHANGE_PAD = 64  # LSCQP_PLAN_EXCHANGE_PAD


def exchange_schedule(n_total, first, count, per=1, pad_agents=None):
    """lscqp_exchange_schedule[_padded]: the collective operations of the exchange that follows a sharded replan (what lscqp_plan_group_step
    runs over RCCL), for blocks [first[g], first[g] + count[g]) of n_total agents, `per` doubles per agent; pad_agents: agents of room
    behind the mission in every device's buffer (None: the unpadded entry).  No device needed."""
    first, count = np.ascontiguousarray(first, dtype=np.int64), np.ascontiguousarray(count, dtype=np.int64)
    ops = np.zeros(max(len(first), 1), EXCHANGE_OP_DTYPE)
    n = C.c_int32()
    if pad_agents is not None:
        _call("lscqp_exchange_schedule_padded", int(n_total), len(first), first, count, int(per), int(pad_agents), ops, len(ops), C.byref(n))
    else:
        _call("lscqp_exchange_schedule", int(n_total), len(first), first, count, int(per), ops, len(ops), C.byref(n))
    return ops[: n.value]


class Comm:
    """lscqp_comm: one host process driving the GPUs of a node (private stream + staging pool + RCCL communicator per device)."""

    def __init__(self, n_devices=0, device_ids=None):
        self._h = C.c_void_p()
        ids = None if device_ids is None else np.ascontiguousarray(device_ids, dtype=np.int32)
        _call("lscqp_comm_create", int(n_devices), ids, C.byref(self._h))
        self.size = lib().lscqp_comm_size(self._h)
        self.backend = lib().lscqp_comm_backend(self._h).decode()

    def close(self):
        if self._h:
            lib().lscqp_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_min_agents_per_device(self, n):
        _call("lscqp_comm_set_min_agents_per_device", self._h, int(n))

    def devices_for(self, n):
        return lib().lscqp_comm_devices_for(self._h, int(n))

    def devices_for_class(self, solver, n, n_obs_max):
        solver._sync_knobs()
        return lib().lscqp_comm_devices_for_class(self._h, solver._h, int(n), int(n_obs_max))

    def prepare(self, solver):
        """lscqp_comm_prepare: the solver's active-set tables on every device of the communicator."""
        _call("lscqp_comm_prepare", self._h, solver._h)

    def stream(self, g):
        return lib().lscqp_comm_stream(self._h, g)

    def synchronize(self):
        _call("lscqp_comm_synchronize", self._h)

    def plan_group_step(self, plans, graph=False):
        """lscqp_plan_group_step: plans[g] lives on device g and owns its block of the mission's agents; every plan's replan is
        enqueued on its device's stream, followed by the in-place RCCL exchange of the owners' plan / state / goal slices."""
        if len(plans) != self.size:
            raise ValueError("one plan per device of the communicator")
        arr = (C.c_void_p * self.size)(*[p._p.value for p in plans])
        _call("lscqp_plan_group_step", self._h, arr, int(bool(graph)))

    def allgather(self, send, recv, count):
        """send / recv: lists of torch CUDA tensors, one per device (device g contributes send[g][:count] doubles and
        receives size * count); asynchronous on the communicator's streams."""
        vp = C.c_void_p * self.size
        ps = vp(*[t.data_ptr() for t in send])
        pr = vp(*[t.data_ptr() for t in recv])
        _call("lscqp_allgather", self._h, ps, pr, int(count))


# The library reads its environment when a handle is CREATED and never afterwards (csrc/lscqp_api.hip: Knobs).  The test suite and bench.py
# flip these switches between launches of one process, on live handles: this wrapper (test and bench plumbing, not the product) notices a change
# of the process environment and tells the handle to re-read it through the library-internal lscqp_debug_reload_knobs_.
_KNOB_ENV = ("LSCQP_FORCE_GENERIC", "LSCQP_WAVES", "LSCQP_ACTIVE_SET", "LSCQP_ACTIVE_SET_NOW", "LSCQP_CHECK_ORDER", "LSCQP_NO_QUEUE", "LSCQP_DEFER_BEHIND", "LSCQP_ZERO_COPY_BYTES")


def _knob_env():
    g = os.environ.get
    return tuple(g(k) for k in _KNOB_ENV)


class Solver:
    def __init__(self, desc):
        self.desc = desc
        self._h = C.c_void_p()
        self._knob_seen = _knob_env()
        _call("lscqp_create", C.byref(desc), C.byref(self._h))
        self.nv = lib().lscqp_num_variables(self._h)
        self.M, self.dim, self.P = desc.M, desc.dim, desc.M * 6

    def _sync_knobs(self):
        now = _knob_env()
        if now != self._knob_seen:
            self._knob_seen = now
            lib().lscqp_debug_reload_knobs_(self._h)

    def set_knob(self, name, value):
        """lscqp_debug_set_knob_ (library-internal): one of the handle's development switches by name, e.g. the launch-shape overrides of
        the dual active-set phase (das_threads, das_kmax, das_steps, das_cache, das_stage, das_screen, das_loop; -1 = the policy's value)."""
        _call("lscqp_debug_set_knob_", self._h, name.encode(), int(value))

    def prepare_device(self):
        _call("lscqp_prepare_device", self._h)

    def bind_device(self, n, n_obs_max, d_hdr, d_rows, d_off, d_sfc, d_x, d_obj, d_status, d_info=None, stream=None, d_x_init=None, retry=False,
                    d_order=None):
        """solve_device with every argument converted ONCE: returns a zero-argument callable that enqueues the same
        lscqp_solve_batch_device_ordered call on the same stream each time it is called (a timed loop then pays for the C entry, not for
        building eleven ctypes pointers per step).  The tensors must stay alive and in place."""
        import torch

        self._sync_knobs()
        s = stream if stream is not None else torch.cuda.current_stream()
        p = _arg
        fn = lib().lscqp_solve_batch_device_ordered
        args = (self._h, n, n_obs_max, p(d_hdr), p(d_rows), p(d_off), p(d_sfc), p(d_x_init), p(d_x), p(d_obj), p(d_status), p(d_info), int(retry),
                p(d_order), C.c_void_p(s.cuda_stream))
        keep = (d_hdr, d_rows, d_off, d_sfc, d_x, d_obj, d_status, d_info, d_x_init, d_order, s)

        def call(_fn=fn, _args=args, _keep=keep):
            rc = _fn(*_args)
            if rc != OK:
                raise LscqpError(rc, lib().lscqp_last_error().decode())

        return call

    def rows_in_format(self, rows):
        """Packed rows (ROW_DTYPE or ROW_F32_DTYPE) in the handle's storage format; fp64 rows are rounded to float32 for
        a ROWS_F32 handle (what a producer writing that format would store)."""
        rows = np.asarray(rows)
        want = ROW_F32_DTYPE if self.desc.row_format == ROWS_F32 else ROW_DTYPE
        if rows.dtype != want:
            src = np.ascontiguousarray(rows, dtype=ROW_DTYPE if rows.dtype.names is None else rows.dtype).reshape(-1)
            out = np.zeros(src.shape, want)
            for f in ("nx", "ny", "nz", "b"):
                out[f] = src[f]
            rows = out
        return np.ascontiguousarray(rows).reshape(-1)

    def close(self):
        if self._h:
            lib().lscqp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, desc):
        _call("lscqp_update", self._h, C.byref(desc))
        self.desc = desc

    def max_obstacles(self):
        return lib().lscqp_max_obstacles(self._h)

    def instance_work(self, n, n_obs_max):
        """lscqp_instance_work: work counters (from the machine code) of the kernel instance a launch of n QPs would select."""
        self._sync_knobs()
        w = Work()
        _call("lscqp_instance_work", self._h, int(n), int(n_obs_max), C.byref(w))
        return {f: (getattr(w, f).decode() if f == "kernel" else getattr(w, f)) for f, _ in Work._fields_}

    def algorithmic_bytes(self, n_obs):
        return lib().lscqp_algorithmic_bytes(self._h, n_obs)

    def num_inequalities(self, n_obs):
        return lib().lscqp_num_inequalities(self._h, n_obs)

    # ---- host-pointer call (numpy) --------------------------------------------------------------------
    def solve_host(self, hdr, rows=None, row_offsets=None, sfc=None, want_info=True, x_init=None):
        """x_init: (n, nv) initial trajectories (TrajOptimizer::solve's initial_traj) as the primal start, or None."""
        self._sync_knobs()
        n = len(hdr)
        hdr = np.ascontiguousarray(hdr, dtype=HEADER_DTYPE)
        x = np.zeros((n, self.nv))
        obj = np.zeros(n)
        status = np.full(n, -1, dtype=np.int32)
        info = np.zeros(n, INFO_DTYPE) if want_info else None
        if rows is not None:
            rows = self.rows_in_format(rows)
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
            assert len(row_offsets) == n + 1
        if sfc is not None:
            sfc = np.ascontiguousarray(sfc, dtype=BOX_DTYPE).reshape(-1)
        if x_init is not None:
            x_init = np.ascontiguousarray(x_init, dtype=np.float64).reshape(n, self.nv)
        _call("lscqp_solve_batch", self._h, n, hdr, rows, row_offsets, sfc, x_init, x, obj, status, info)
        return dict(x=x, obj=obj, status=status, info=info)

    def solve_sharded(self, comm, hdr, rows=None, row_offsets=None, sfc=None, want_info=True, x_init=None):
        """lscqp_solve_batch_sharded: the host-pointer call over the devices of `comm`; returns solve_host's dict + devices_used."""
        self._sync_knobs()
        n = len(hdr)
        hdr = np.ascontiguousarray(hdr, dtype=HEADER_DTYPE)
        x = np.zeros((n, self.nv))
        obj = np.zeros(n)
        status = np.full(n, -1, dtype=np.int32)
        info = np.zeros(n, INFO_DTYPE) if want_info else None
        if rows is not None:
            rows = self.rows_in_format(rows)
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        if sfc is not None:
            sfc = np.ascontiguousarray(sfc, dtype=BOX_DTYPE).reshape(-1)
        if x_init is not None:
            x_init = np.ascontiguousarray(x_init, dtype=np.float64).reshape(n, self.nv)
        used = C.c_int32(0)
        _call("lscqp_solve_batch_sharded", self._h, comm._h, n, hdr, rows, row_offsets, sfc, x_init, x, obj, status, info, C.cast(C.byref(used), C.c_void_p))
        return dict(x=x, obj=obj, status=status, info=info, devices_used=used.value)

    # ---- failure diagnostics (include/lscqp.h) -------------------------------------------------------------
    def diagnose_host(self, hdr, rows, row_offsets, sfc, x, tol=1e-9):
        """lscqp_diagnose: every row of the reference's model evaluated on the trajectories x (n, nv) -> DIAG_DTYPE[n]."""
        n = len(hdr)
        hdr = np.ascontiguousarray(hdr, dtype=HEADER_DTYPE)
        out = np.zeros(n, DIAG_DTYPE)
        if rows is not None:
            rows = self.rows_in_format(rows)
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        if sfc is not None:
            sfc = np.ascontiguousarray(sfc, dtype=BOX_DTYPE).reshape(-1)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(n, self.nv)
        _call("lscqp_diagnose", self._h, n, hdr, rows, row_offsets, sfc, x, float(tol), out)
        return out

    def dump_instance(self, hdr_one, rows_one, sfc_one, path):
        """lscqp_dump_instance: ONE instance as a CPLEX LP file (what cplex.exportModel writes in the reference); needs no device."""
        hdr = np.ascontiguousarray(hdr_one, dtype=HEADER_DTYPE).reshape(1)
        rows = None if rows_one is None else self.rows_in_format(rows_one)
        sfc = None if sfc_one is None else np.ascontiguousarray(sfc_one, dtype=BOX_DTYPE).reshape(-1)
        _call("lscqp_dump_instance", self._h, hdr, rows, sfc, os.fsencode(path))

    def solve_sharded_device(self, comm, n, n_obs_max, d_hdr, d_rows, d_off, d_sfc, d_x, d_obj, d_status, d_info=None, d_x_init=None, retry=False):
        """lscqp_solve_batch_sharded_device: lists of per-device torch CUDA tensors (entry g lives on device g of `comm`), n[g] agents on
        device g; asynchronous on the communicator's streams (comm.synchronize() waits)."""
        self._sync_knobs()
        G = comm.size
        vp = C.c_void_p * G

        def arr(ts):
            return None if ts is None else vp(*[(None if t is None else t.data_ptr()) for t in ts])

        nn = (C.c_int64 * G)(*[int(v) for v in n])
        _call("lscqp_solve_batch_sharded_device", self._h, comm._h, nn, int(n_obs_max), arr(d_hdr), arr(d_rows), arr(d_off), arr(d_sfc), arr(d_x_init),
              arr(d_x), arr(d_obj), arr(d_status), arr(d_info), int(bool(retry)))

    # ---- device-pointer call (torch tensors hold the HBM buffers) --------------------------------------
    def solve_device(self, n, n_obs_max, d_hdr, d_rows, d_off, d_sfc, d_x, d_obj, d_status, d_info=None, stream=None,
                     d_x_init=None, retry=False, d_order=None):
        """All arguments are torch CUDA tensors (any dtype; only data_ptr() is used) or None.
        Asynchronous on `stream` (torch.cuda.Stream) or torch's current stream.  retry: lscqp_solve_batch_device_ex's second pass.
        d_order: int32 permutation of 0 .. n-1 (lscqp_solve_batch_device_ordered: the k-th slot of the launch solves instance d_order[k])."""
        self._sync_knobs()
        _call("lscqp_solve_batch_device_ordered", self._h, n, n_obs_max, d_hdr, d_rows, d_off, d_sfc, d_x_init, d_x, d_obj, d_status, d_info, int(retry),
              d_order, stream=stream)

    # ---- the prescreen (include/lscqp.h) --------------------------------------------------------------------
    def set_prescreen(self, mode):
        """lscqp_set_prescreen: PRESCREEN_ON / PRESCREEN_OFF -- the per-control-point infeasibility test in front of every solve of this handle."""
        _call("lscqp_set_prescreen", self._h, int(mode))

    def prescreen(self):
        return lib().lscqp_prescreen(self._h)

    def prescreen_device(self, n, n_obs_max, d_hdr, d_rows, d_off, d_sfc, d_cert, stream=None):
        """lscqp_prescreen_batch_device: the test alone, one PRESCREEN_CERT_DTYPE record per instance into d_cert (72 n bytes).  Torch CUDA
        tensors (only data_ptr() is used) or None; asynchronous on `stream` or torch's current stream."""
        _call("lscqp_prescreen_batch_device", self._h, n, n_obs_max, d_hdr, d_rows, d_off, d_sfc, d_cert, stream=stream)

    def prescreen_host(self, hdr, rows, row_offsets, sfc):
        """The prescreen on host arrays: staged to the current device, tested there, the certificates (PRESCREEN_CERT_DTYPE[n]) fetched back."""
        import torch

        n = len(hdr)
        hdr = np.ascontiguousarray(hdr, dtype=HEADER_DTYPE)
        n_obs_max = int(hdr["n_obs"].max()) if n else 0
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None

        def up(a):
            if a is None:
                return None
            t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())
            return t.to(dev) if dev is not None else t

        d_rows = up(self.rows_in_format(rows)) if rows is not None else None
        d_off = up(np.ascontiguousarray(row_offsets, dtype=np.uint64)) if row_offsets is not None else None
        d_sfc = up(np.ascontiguousarray(sfc, dtype=BOX_DTYPE).reshape(-1)) if sfc is not None else None
        d_hdr = up(hdr)
        d_cert = torch.zeros(max(n, 1) * PRESCREEN_CERT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.prescreen_device(n, max(n_obs_max, 0), d_hdr, d_rows, d_off, d_sfc, d_cert)
        torch.cuda.synchronize()
        return d_cert.cpu().numpy()[:n * PRESCREEN_CERT_DTYPE.itemsize].view(PRESCREEN_CERT_DTYPE).copy()

    def prescreen_twin(self, hdr, rows, row_offsets, sfc, n_obs_max=None):
        """(library-internal, tests) the prescreen kernel's per-control-point arithmetic on the host: lscqp_debug_prescreen_twin_."""
        n = len(hdr)
        hdr = np.ascontiguousarray(hdr, dtype=HEADER_DTYPE)
        rows = self.rows_in_format(rows) if rows is not None else None
        row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64) if row_offsets is not None else None
        sfc = np.ascontiguousarray(sfc, dtype=BOX_DTYPE).reshape(-1) if sfc is not None else None
        out = np.zeros(n, PRESCREEN_CERT_DTYPE)
        cap = int(hdr["n_obs"].max()) if n_obs_max is None else int(n_obs_max)
        _call("lscqp_debug_prescreen_twin_", self._h, n, max(cap, 0), hdr, rows, row_offsets, sfc, out)
        return out

    def solve_plan(self, n, n_obs_max, retry=0, part=PLAN_WHOLE, has_x_init=False, has_order=False, deferred=False, n_cu=256, tables_available=True):
        """(library-internal, tests) what a solve call of this handle WOULD launch: lscqp_debug_solve_plan_, the very planner the solve worker
        runs, on no device.  {"passes": [...], "deferred", "error", "capacity"}; a pass of kind "fused" is followed by the "phase" and the
        "instance" pass that run in its place when the fused launcher refuses the budgets."""
        self._sync_knobs()
        out = _Plan()
        _call("lscqp_debug_solve_plan_", self._h, int(n), int(n_obs_max), int(retry), int(part), int(has_x_init), int(has_order), int(deferred), int(n_cu),
              int(tables_available), C.byref(out))
        passes = []
        for ps in out.passes[:out.n_pass]:
            d = {k: getattr(ps, k) for k, _ in _PlanPass._fields_ if k != "inst"}
            d["kind"], d["what"] = PLAN_PASS_KINDS[ps.kind], ps.what.decode()
            if d["kind"] in ("phase", "fused"):  # the launch shape of the phase
                d.update({k: getattr(out.phase, k) for k, _ in _PlanPhase._fields_})
            passes.append(d)
        return {"passes": passes, "deferred": bool(out.deferred), "error": PLAN_ERRORS[out.error], "capacity": out.capacity}

    def device_fill(self, n, n_obs_max):
        """lscqp_device_fill: instances one device works on at once in the first kernel of a solve of this class."""
        self._sync_knobs()
        return lib().lscqp_device_fill(self._h, int(n), int(n_obs_max))

    def launch_capacity(self, n, n_obs_max):
        """lscqp_launch_capacity: instances of a launch of n the device works on at once (-1 without a device)."""
        self._sync_knobs()
        return int(lib().lscqp_launch_capacity(self._h, int(n), int(n_obs_max)))

    @staticmethod
    def order_by_cost_device(n, d_cost_prev, d_order_out, stream=None):
        """lscqp_order_by_cost_device: d_order_out (int32[n]) := agents by the cost (uint32) of their previous corridor, most expensive first."""
        _call("lscqp_order_by_cost_device", int(n), d_cost_prev, d_order_out, stream=stream)

    @staticmethod
    def order_by_work_device(n, d_info_prev, d_order_out, stream=None):
        """lscqp_order_by_work_device: d_order_out (int32[n]) := instances by the iterations of their previous solve, most first."""
        _call("lscqp_order_by_work_device", int(n), d_info_prev, d_order_out, stream=stream)

    # ---- GoalOptimizer::solve in closed form ----------------------------------------
    def optimize_goal_host(self, hdr, rows=None, row_offsets=None, sfc=None):
        """hdr["goal"] = current_goal_point on entry; returns (hdr with the optimised goal, status)."""
        n = len(hdr)
        hdr = np.ascontiguousarray(hdr, dtype=HEADER_DTYPE).copy()
        status = np.full(n, -1, dtype=np.int32)
        if rows is not None:
            rows = self.rows_in_format(rows)
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        if sfc is not None:
            sfc = np.ascontiguousarray(sfc, dtype=BOX_DTYPE).reshape(-1)
        _call("lscqp_optimize_goal", self._h, n, hdr, rows, row_offsets, sfc, status)
        return hdr, status

    def optimize_goal_device(self, n, d_hdr, d_rows, d_off, d_sfc, d_status, stream=None):
        _call("lscqp_optimize_goal_device", self._h, n, d_hdr, d_rows, d_off, d_sfc, d_status, stream=stream)

    def optimize_goal_fin_device(self, n, d_hdr, d_rows, d_off, d_sfc, d_status, fin_dt, stream=None):
        """(library-internal, tests) lscqp_optimize_goal_fin_device_: the goal LP as the replan chain runs it -- the goal left as a point3d
        (float32 values) and terminal_segments written from it (fin_dt = the class's dt)."""
        _call("lscqp_optimize_goal_fin_device_", self._h, n, d_hdr, d_rows, d_off, d_sfc, d_status, float(fin_dt), stream=stream)

    # ---- isSolValid + getStateAt + doStep -------------------------------------------
    def safety_metrics_device(self, n_agents, first_agent, n_total, n_samples, record_time_step, d_x_all, d_radius, d_downwash, d_hdr,
                              d_out, z_2d=1.0, stream=None):
        """MultiSyncSimulator::update's safety ratio / excess ratios per local agent (SAFETY_DTYPE records in d_out)."""
        _call("lscqp_safety_metrics_device", self._h, n_agents, first_agent, n_total, int(n_samples), float(record_time_step), float(z_2d), d_x_all,
              d_radius, d_downwash, d_hdr, d_out, stream=stream)

    def safety_obstacles_device(self, n_agents, first_agent, n_total, n_samples, record_time_step, d_x_all, d_radius, d_downwash, n_obstacles,
                                d_obstacles, d_out, z_2d=1.0, stream=None):
        """MultiSyncSimulator::update's obstacle safety ratio per local agent (SAFETY_OBS_DTYPE records in d_out; d_obstacles: OBSTACLE_DTYPE)."""
        _call("lscqp_safety_obstacles_device", self._h, n_agents, first_agent, n_total, int(n_samples), float(record_time_step), float(z_2d), d_x_all,
              d_radius, d_downwash, int(n_obstacles), d_obstacles, d_out, stream=stream)

    def safety_obstacles_ids_device(self, n_agents, first_agent, n_total, n_samples, record_time_step, d_x_all, d_radius, d_downwash, n_slots,
                                    d_obstacle_ids, n_obstacles, d_obstacles, d_out, z_2d=1.0, stream=None):
        """lscqp_safety_obstacles_ids_device: safety_obstacles_device with each local agent's own obstacles, row a of d_obstacle_ids
        (int32 (n_agents, n_slots): table indices, < 0 = none); closest_obstacle is the slot."""
        _call("lscqp_safety_obstacles_ids_device", self._h, n_agents, first_agent, n_total, int(n_samples), float(record_time_step), float(z_2d), d_x_all,
              d_radius, d_downwash, int(n_slots), d_obstacle_ids, int(n_obstacles), d_obstacles, d_out, stream=stream)

    def construct_sfc_device(self, world_map, mode, n, d_points, d_radius, d_sfc, d_status, stream=None, d_order=None, d_cost=None):
        """Corridor update of n agents on the device (SFC_INIT / SFC_FROM_HULL / SFC_FROM_POINT, see include/lscqp.h).  d_order: int32
        permutation (workgroup k builds agent d_order[k]'s corridor); d_cost: uint32[n], every agent's cost of this launch."""
        _call("lscqp_construct_sfc_device_ordered", self._h, world_map._h, int(mode), n, d_points, d_radius, d_sfc, d_status, d_order, d_cost, stream=stream)

    def construct_sfc_worlds_device(self, worlds, mode, n, d_world_of, d_points, d_radius, d_sfc, d_status, stream=None, d_order=None, d_cost=None):
        """lscqp_construct_sfc_worlds_device: construct_sfc_device in which agent a is tested against world d_world_of[a] (int32 (n,)) of a
        Worlds set; every index must lie in [0, len(worlds))."""
        _call("lscqp_construct_sfc_worlds_device", self._h, worlds._w, int(mode), n, d_world_of, d_points, d_radius, d_sfc, d_status, d_order, d_cost,
              stream=stream)

    def validate_step_device(self, n, time_step, d_x, d_hdr, d_sfc, d_valid, d_state, z_2d=1.0, stream=None):
        _call("lscqp_validate_step_device", self._h, n, float(time_step), float(z_2d), d_x, d_hdr, d_sfc, d_valid, d_state, stream=stream)

    def commit_validate_device(self, n, time_step, d_qp_status, d_x_new, d_x_init, d_x_plan, d_goal, d_hdr, d_sfc, d_valid, d_state, z_2d=1.0,
                               stream=None):
        """(library-internal, tests) lscqp_commit_validate_raw_: the replan chain's commit (x_plan = x_new where the QP is OPTIMAL, else
        x_init; goal = hdr.goal) with isSolValid + doStep on the plan it chose, in one launch."""
        d = self.desc
        _call("lscqp_commit_validate_raw_", int(d.M), int(d.dim), int(d.use_sfc), float(d.dt), n, float(time_step), float(z_2d), d_qp_status, d_x_new,
              d_x_init, d_x_plan, d_goal, d_hdr, d_sfc, d_valid, d_state, stream=stream)

    # ---- the producer of the rows, device pointers -----------------------------------
    def generate_lsc_device(self, n_agents, n_obs, first_agent, d_traj, d_neighbours, d_radius, d_downwash, d_goal, d_rows,
                            stream=None):
        """TrajPlanner::generateLSC for agent obstacles, rows written in the layout solve_device consumes."""
        _call("lscqp_generate_lsc_device", self._h, n_agents, n_obs, first_agent, d_traj, d_neighbours, d_radius, d_downwash, d_goal, d_rows, stream=stream)

    def generate_constraints_device(self, mode, n_agents, n_obs, first_agent, d_traj, d_neighbours, d_radius, d_downwash, d_goal_all,
                                    d_rows, stream=None):
        """generateLSC / generateCLSC / generateBVC (mode GEN_LSC / GEN_CLSC / GEN_BVC) on the device; d_goal_all holds the
        current goal point of every agent, indexed by global id (see include/lscqp.h)."""
        _call("lscqp_generate_constraints_device", self._h, int(mode), n_agents, n_obs, first_agent, d_traj, d_neighbours, d_radius, d_downwash, d_goal_all,
              d_rows, stream=stream)

    def select_neighbours_device(self, n_agents, first_agent, n_total, n_obs, comm_range, d_positions, d_neighbours, d_count, stream=None):
        """broadcastMsgs' range filter on the device: neighbour ids (ascending, -1 padded) and the in-range counts."""
        _call("lscqp_select_neighbours_device", self._h, n_agents, first_agent, n_total, int(n_obs), float(comm_range), d_positions, d_neighbours, d_count,
              stream=stream)

    def select_neighbours_missions_device(self, offsets, n_obs, comm_range, d_positions, d_neighbours, d_count, stream=None):
        """select_neighbours_device with the agent's own mission of the partition `offsets` (host, [K + 1]) as its candidates."""
        K, off, d_off = mission_offsets_arg(offsets, d_positions.device)
        s = _call("lscqp_select_neighbours_missions_device", self._h, int(off[-1]), K, off, d_off, int(n_obs), float(comm_range), d_positions, d_neighbours,
                  d_count, stream=stream)
        s.synchronize()  # (d_off is this call's own)

    def safety_metrics_missions_device(self, offsets, n_samples, record_time_step, d_x_all, d_radius, d_downwash, d_hdr, d_out, z_2d=1.0, stream=None):
        """safety_metrics_device over the pairs within each mission of the partition `offsets` (host, [K + 1])."""
        K, off, d_off = mission_offsets_arg(offsets, d_x_all.device)
        s = _call("lscqp_safety_metrics_missions_device", self._h, int(off[-1]), K, off, d_off, int(n_samples), float(record_time_step), float(z_2d), d_x_all,
                  d_radius, d_downwash, d_hdr, d_out, stream=stream)
        s.synchronize()

    def shift_traj_device(self, n, d_x_prev, d_traj, z_2d=1.0, shift=1, stream=None):
        """initialTrajPlanningPrevSol: solver output [n][dim*M*6] -> initial trajectories [n][M][6][3] (float32 values)."""
        _call("lscqp_shift_traj_device", self._h, n, int(shift), float(z_2d), d_x_prev, d_traj, stream=stream)

    def shift_traj_partial_device(self, n, d_x_prev, d_traj, fraction, z_2d=1.0, stream=None):
        """multisim_time_step < dt: segment 0 := subSegment(fraction, 1) of the previous plan's, the others kept."""
        _call("lscqp_shift_traj_partial_device", self._h, n, float(fraction), float(z_2d), d_x_prev, d_traj, stream=stream)

    def generate_constraints_device_ex(self, mode, n_agents, n_obs, first_agent, d_traj, d_neighbours, d_radius, d_downwash, d_goal_all,
                                       d_rows, n_obs_total, slot0, stream=None):
        _call("lscqp_generate_constraints_device_ex", self._h, int(mode), n_agents, n_obs, first_agent, d_traj, d_neighbours, d_radius, d_downwash,
              d_goal_all, d_rows, int(n_obs_total), int(slot0), stream=stream)

    def generate_lsc_obstacles_device(self, param, n_agents, n_dyn, first_agent, d_traj, d_ids, d_obstacles, d_radius, d_goal, d_hdr, d_rows,
                                      n_obs_total, slot0, stream=None):
        """generateLSC for non-agent obstacles (param: ObstacleParam; d_obstacles: OBSTACLE_DTYPE table on the device)."""
        _call("lscqp_generate_lsc_obstacles_device", self._h, C.cast(C.byref(param), C.c_void_p), n_agents, n_dyn, first_agent, d_traj, d_ids, d_obstacles,
              d_radius, d_goal, d_hdr, d_rows, int(n_obs_total), int(slot0), stream=stream)

    def generate_obstacle_rows_device(self, mode, param, n_agents, n_dyn, first_agent, d_traj, d_ids, d_obstacles, d_obstacle_goal, d_radius, d_goal,
                                      d_hdr, d_rows, n_obs_total, slot0, stream=None):
        """The rows of non-agent obstacles by generator: GEN_LSC is generate_lsc_obstacles_device, GEN_CLSC generateCLSC's non-agent branch
        (d_obstacle_goal: [table][3] goal points or None = the origin; d_hdr may be None)."""
        _call("lscqp_generate_obstacle_rows_device", self._h, int(mode), C.cast(C.byref(param), C.c_void_p), n_agents, n_dyn, first_agent, d_traj, d_ids,
              d_obstacles, d_obstacle_goal, d_radius, d_goal, d_hdr, d_rows, int(n_obs_total), int(slot0), stream=stream)

    def obstacles_advance_device(self, d_models, n_dyn, time_step, d_clock, d_obstacles, stream=None):
        """lscqp_obstacles_advance_device: the table moved to the clock's replan, the clock advanced; d_models PREPARED models on the device."""
        _call("lscqp_obstacles_advance_device", self._h, d_models, int(n_dyn), float(time_step), d_clock, d_obstacles, stream=stream)

    def obstacles_advance_missions_device(self, d_models, obstacle_offsets, d_obstacle_offsets, time_step, d_clock, d_obstacles, stream=None):
        """lscqp_obstacles_advance_missions_device: obstacles_advance_device over a mission-major table, one workgroup and one word of
        d_clock (int32 (K,)) per mission.  obstacle_offsets: int32 (K + 1,) on the host, d_obstacle_offsets the same on the device."""
        off = np.ascontiguousarray(obstacle_offsets, dtype=np.int32)
        _call("lscqp_obstacles_advance_missions_device", self._h, d_models, len(off) - 1, off, d_obstacle_offsets, int(off[-1]), float(time_step), d_clock,
              d_obstacles, stream=stream)

    def obstacles_drive_missions_device(self, d_models, d_drives, obstacle_offsets, d_obstacle_offsets, d_acc_history, n_history, d_state, n_total,
                                        d_drive_state, time_step, d_clock, d_obstacles, stream=None):
        """lscqp_obstacles_drive_missions_device: obstacles_drive_device over a mission-major table, one workgroup per mission over its own
        slice, IN FRONT of obstacles_advance_missions_device (d_clock int32 (K,) is read, not advanced)."""
        off = np.ascontiguousarray(obstacle_offsets, dtype=np.int32)
        _call("lscqp_obstacles_drive_missions_device", self._h, d_models, d_drives, len(off) - 1, off, d_obstacle_offsets, int(off[-1]), d_acc_history,
              int(n_history), d_state, int(n_total), d_drive_state, float(time_step), d_clock, d_obstacles, stream=stream)

    def obstacles_drive_device(self, d_models, d_drives, n_dyn, d_acc_history, n_history, d_state, n_total, d_drive_state, time_step, d_clock,
                               d_obstacles, stream=None):
        """lscqp_obstacles_drive_device: the chasing and gaussian entries of the table moved to the clock's replan, IN FRONT of
        obstacles_advance_device on the same stream (the clock is read, not advanced).  d_drives: OBSTACLE_DRIVE_DTYPE, d_drive_state:
        OBSTACLE_DRIVE_STATE_DTYPE per obstacle, zeroed before the first replan; d_state [n_total][9]."""
        _call("lscqp_obstacles_drive_device", self._h, d_models, d_drives, int(n_dyn), d_acc_history, int(n_history), d_state, int(n_total), d_drive_state,
              float(time_step), d_clock, d_obstacles, stream=stream)

    def obstacle_drive_host(self, models, drives, acc_history, state, drive_state, time_step, clock, table):
        """lscqp_obstacle_drive_host: one replan of the drives on the CPU, by the functions the kernel runs; numpy arrays, `drive_state`
        (OBSTACLE_DRIVE_STATE_DTYPE) and `table` (OBSTACLE_DTYPE) are written in place; `clock` is the replan index.  No device needed."""
        m, d = np.ascontiguousarray(models, dtype=OBSTACLE_MODEL_DTYPE), np.ascontiguousarray(drives, dtype=OBSTACLE_DRIVE_DTYPE)
        h = np.ascontiguousarray(np.zeros((0, 3)) if acc_history is None else acc_history, dtype=np.float64).reshape(-1, 3)
        st = np.ascontiguousarray(np.zeros((0, 9)) if state is None else state, dtype=np.float64).reshape(-1, 9)
        for a, dt in ((drive_state, OBSTACLE_DRIVE_STATE_DTYPE), (table, OBSTACLE_DTYPE)):
            if a.dtype != dt or not a.flags.c_contiguous or len(a) != len(d):
                raise ValueError("drive_state and table are written in place: contiguous arrays of their dtypes, one record per drive")
        _call("lscqp_obstacle_drive_host", self._h, m, d, len(d), h if len(h) else None, len(h), st if len(st) else None, len(st), drive_state,
              float(time_step), np.array([clock], np.int32), table, None)

    def patrol_device(self, n, d_state, d_desired, d_start, goal_threshold, dim, z_2d, d_legs, d_swapped, stream=None):
        """lscqp_patrol_device: the PATROL transition of n agents; d_desired / d_start [n][3] float64 are swapped in place where an agent has
        arrived, d_legs incremented, d_swapped written (1 / 0) for every agent."""
        _call("lscqp_patrol_device", self._h, int(n), d_state, d_desired, d_start, float(goal_threshold), int(dim), float(z_2d), d_legs, d_swapped, stream=stream)

    def patrol_host(self, state, desired, start, goal_threshold, dim, z_2d, legs, swapped):
        """lscqp_patrol_host: the same on the CPU, by the function the kernel runs; `desired`, `start` (float64 (n, 3)), `legs` and `swapped`
        (int32 (n,)) are written in place.  No device needed."""
        st = np.ascontiguousarray(state, dtype=np.float64).reshape(-1, 9)
        for a, dt, per in ((desired, np.float64, 3), (start, np.float64, 3), (legs, np.int32, 1), (swapped, np.int32, 1)):
            if a.dtype != dt or not a.flags.c_contiguous or a.size != len(st) * per:
                raise ValueError("desired, start, legs and swapped are written in place: contiguous arrays of their dtypes, one entry per agent")
        _call("lscqp_patrol_host", self._h, len(st), st if len(st) else None, desired, start, float(goal_threshold), int(dim), float(z_2d), legs, swapped, None)

    @staticmethod
    def field_exchange_device(n, nodes, d_swapped, d_field, d_field_other, d_init_d, d_init_d_other, stream=None):
        """lscqp_field_exchange_device: the slices [a * nodes, (a + 1) * nodes) of the two int32 fields, and the two init_d words, exchanged
        for every agent with d_swapped[a] == 1."""
        _call("lscqp_field_exchange_device", int(n), int(nodes), d_swapped, d_field, d_field_other, d_init_d, d_init_d_other, stream=stream)

    def generate_lsc_bytes(self, n_agents, n_obs, n_total):
        return lib().lscqp_generate_lsc_bytes(self._h, n_agents, n_obs, n_total)


def x_init_from_swarm(build, dim):
    """synth.Swarm.build()["init"] (N, M, 6, 3) -> (N, dim*M*6) in the reference variable order (axis, segment, point)."""
    init = np.asarray(build["init"], dtype=np.float64)
    N = init.shape[0]
    return np.ascontiguousarray(init.transpose(0, 3, 1, 2)[:, :dim]).reshape(N, -1)


def batch_from_swarm(build, n_obs, M, vmax=1.0, amax=2.0, radius=0.15, nominal_velocity=1.0, terminal_segments=None):
    """Pack the output of synth.Swarm.build() into ABI arrays (hdr, rows, row_offsets, sfc)."""
    N = len(build["p0"])
    hdr = np.zeros(N, HEADER_DTYPE)
    for f in ("p0", "v0", "a0", "goal", "next_waypoint"):
        hdr[f] = build[f]
    hdr["vmax"], hdr["amax"] = vmax, amax
    hdr["radius"], hdr["nominal_velocity"] = radius, nominal_velocity
    hdr["n_obs"] = n_obs
    hdr["terminal_segments"] = 0 if terminal_segments is None else terminal_segments
    rows = pack_rows(build["lsc"]).reshape(-1)
    off = (np.arange(N + 1, dtype=np.uint64) * np.uint64(n_obs * M * 6))
    sfc = np.zeros((N, M), BOX_DTYPE)
    sfc["bmin"], sfc["bmax"] = build["sfc"]["bmin"], build["sfc"]["bmax"]
    return hdr, rows, off, sfc
