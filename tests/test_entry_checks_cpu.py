"""CPU test of the argument checks of the device entries that are defined beside their kernel launch (csrc/lscgen.hip, lscgoal.hip,
lscpost.hip, lscsfc.hip): for every entry a table of calls through api.lib() with plain ctypes -- no torch.cuda -- each with the return
code and the lscqp_last_error() text it must give.  The table pins WHICH check answers and, where a call breaks two checks at once, that
the earlier one does: null handle, then sizes / mode, then the empty batch (LSCQP_OK, even with null buffers and without a device), then
null buffers, then the device.

The expected codes and texts are literals, taken from the library as it was BEFORE the entries moved out of csrc/lscqp_api.hip (the table
was run against that build through LSCQP_LIB); the same table passes on that library and on this one.

Two checks have no row: "obstacle prediction supports M <= 32" and "corridor shift supports M <= 21" sit behind a handle, and
lscqp_create refuses every class with M > 12 (no kernel for it), so no call can reach them.
"""
import ctypes as C

import pytest

OK, INVALID, UNSUPPORTED, NO_DEVICE = 0, 1, 2, 3
NULL_HANDLE, NEGATIVE, NULL_BUFFER, INCONSISTENT = "null handle", "negative size", "null buffer", "inconsistent sizes"
NO_DEVICE_TEXT = "no HIP device: lscqp has no CPU fallback"
GEN_MODE = "mode must be LSCQP_GEN_LSC, LSCQP_GEN_CLSC or LSCQP_GEN_BVC"
SFC_MODE = "mode must be LSCQP_SFC_INIT, LSCQP_SFC_FROM_HULL or LSCQP_SFC_FROM_POINT"
SLOTS = "n_obs_total >= slot0 + n_obs required"
DYN_SLOTS = "inconsistent sizes (n_obs_total >= slot0 + n_dyn required)"
SHIFT = "shift_segments must be 0 or 1"
FRACTION = "fraction = multisim_time_step / dt must lie in (0, 1)"
TIME = "negative size or time"
PART_NEEDS = "a mission partition needs n_missions >= 1 and its offset list"
PART_FIRST = "mission_offsets[0] must be 0"
PART_ORDER = "mission_offsets must be strictly increasing (no empty mission)"
PART_LAST = "mission_offsets[n_missions] must be the number of agents"
NAN = float("nan")

# Values that exist only once the library is loaded are named here and looked up in `world` below: "h" a handle (M = 5, 3-D, corridors on),
# "h_nosfc" one without corridors, "p" some non-null address, "mp" a non-null map address (never followed: every row that is run where a
# device exists ends before the launch), "param" an lscqp_obstacle_param, "off" the host offsets [0, 4, 10] of a partition of 10 agents.
# Per entry: its parameters in order, with arguments that pass every check (the stream, last, is NULL).
GOOD = {
    "lscqp_generate_lsc_device": [("h", "h"), ("n_agents", 1), ("n_obs", 1), ("first_agent", 0), ("d_traj", "p"), ("d_neighbours", "p"),
                                  ("d_radius", "p"), ("d_downwash", "p"), ("d_goal", "p"), ("d_rows_out", "p")],
    "lscqp_generate_constraints_device": [("h", "h"), ("mode", 1), ("n_agents", 1), ("n_obs", 1), ("first_agent", 0), ("d_traj", "p"),
                                          ("d_neighbours", "p"), ("d_radius", "p"), ("d_downwash", "p"), ("d_goal_all", "p"), ("d_rows_out", "p")],
    "lscqp_generate_constraints_device_ex": [("h", "h"), ("mode", 2), ("n_agents", 1), ("n_obs", 2), ("first_agent", 0), ("d_traj", "p"),
                                             ("d_neighbours", "p"), ("d_radius", "p"), ("d_downwash", "p"), ("d_goal_all", "p"),
                                             ("d_rows_out", "p"), ("n_obs_total", 5), ("slot0", 3)],
    "lscqp_generate_constraints_own_": [("h", "h"), ("mode", 0), ("n_agents", 1), ("n_obs", 2), ("first_agent", 0), ("d_traj", "p"),
                                        ("d_own_traj", None), ("d_neighbours", "p"), ("d_radius", "p"), ("d_downwash", "p"), ("d_goal_all", "p"),
                                        ("d_rows_out", "p"), ("n_obs_total", 5), ("slot0", 3)],
    "lscqp_generate_lsc_obstacles_device": [("h", "h"), ("param", "param"), ("n_agents", 1), ("n_dyn", 2), ("first_agent", 0), ("d_traj", "p"),
                                            ("d_obstacle_ids", "p"), ("d_obstacles", "p"), ("d_radius", "p"), ("d_goal", "p"), ("d_hdr", "p"),
                                            ("d_rows_out", "p"), ("n_obs_total", 5), ("slot0", 3)],
    "lscqp_shift_traj_device": [("h", "h"), ("n", 1), ("shift_segments", 1), ("z_2d", 1.0), ("d_x_prev", "p"), ("d_traj", "p")],
    "lscqp_shift_traj_partial_device": [("h", "h"), ("n", 1), ("fraction", 0.5), ("z_2d", 1.0), ("d_x_prev", "p"), ("d_traj", "p")],
    "lscqp_select_neighbours_device": [("h", "h"), ("n_agents", 1), ("first_agent", 2), ("n_total", 3), ("n_obs", 2), ("range", 3.0),
                                       ("d_positions", "p"), ("d_neighbours_out", "p"), ("d_count_out", "p")],
    "lscqp_select_neighbours_missions_device": [("h", "h"), ("n_total", 10), ("n_missions", 2), ("mission_offsets", "off"),
                                                ("d_mission_offsets", "p"), ("n_obs", 2), ("range", 3.0), ("d_positions", "p"),
                                                ("d_neighbours_out", "p"), ("d_count_out", "p")],
    "lscqp_optimize_goal_device": [("h", "h"), ("n", 1), ("d_hdr", "p"), ("d_rows", None), ("d_row_offsets", None), ("d_sfc", "p"),
                                   ("d_status_out", "p")],
    "lscqp_optimize_goal_fin_device_": [("h", "h"), ("n", 1), ("d_hdr", "p"), ("d_rows", None), ("d_row_offsets", None), ("d_sfc", "p"),
                                        ("d_status_out", "p"), ("fin_dt", 0.2)],
    "lscqp_safety_metrics_device": [("h", "h"), ("n_agents", 1), ("first_agent", 2), ("n_total", 3), ("n_samples", 2), ("record_time_step", 0.1),
                                    ("z_2d", 1.0), ("d_x_all", "p"), ("d_radius", "p"), ("d_downwash", "p"), ("d_hdr", "p"), ("d_out", "p")],
    "lscqp_safety_obstacles_device": [("h", "h"), ("n_agents", 1), ("first_agent", 2), ("n_total", 3), ("n_samples", 2), ("record_time_step", 0.1),
                                      ("z_2d", 1.0), ("d_x_all", "p"), ("d_radius", "p"), ("d_downwash", "p"), ("n_obstacles", 2),
                                      ("d_obstacles", "p"), ("d_out", "p")],
    "lscqp_safety_metrics_missions_device": [("h", "h"), ("n_total", 10), ("n_missions", 2), ("mission_offsets", "off"), ("d_mission_offsets", "p"),
                                             ("n_samples", 2), ("record_time_step", 0.1), ("z_2d", 1.0), ("d_x_all", "p"), ("d_radius", "p"),
                                             ("d_downwash", "p"), ("d_hdr", "p"), ("d_out", "p")],
    "lscqp_validate_step_device": [("h", "h"), ("n", 1), ("time_step", 0.2), ("z_2d", 1.0), ("d_x", "p"), ("d_hdr", "p"), ("d_sfc", "p"),
                                   ("d_valid_out", "p"), ("d_state_out", "p")],
    "lscqp_construct_sfc_device": [("h", "h"), ("mp", "mp"), ("mode", 1), ("n", 1), ("d_points", "p"), ("d_radius", "p"), ("d_sfc", "p"),
                                   ("d_status_out", "p")],
    "lscqp_construct_sfc_device_ordered": [("h", "h"), ("mp", "mp"), ("mode", 2), ("n", 1), ("d_points", "p"), ("d_radius", "p"), ("d_sfc", "p"),
                                           ("d_status_out", "p"), ("d_order", None), ("d_cost_out", None)],
}


def _buffers(entry):
    """The parameters of `entry` that must not be NULL when the batch is not empty."""
    optional = {"d_own_traj", "d_rows", "d_row_offsets", "d_order", "d_cost_out"}
    return [k for k, _ in GOOD[entry] if k.startswith("d_") and k not in optional]


def _all_null(entry):
    return {k: None for k in _buffers(entry)}


def _rows():
    """(entry, what is wrong, {parameter: value} over GOOD[entry], return code, lscqp_last_error() or None where the call succeeds)"""
    T = []

    def row(entry, what, change, rc, text):
        assert all(k in dict(GOOD[entry]) for k in change), (entry, what)
        T.append((entry, what, change, rc, text))

    gens = ("lscqp_generate_constraints_device", "lscqp_generate_constraints_device_ex", "lscqp_generate_constraints_own_")
    for e in GOOD:
        # the null handle answers first, whatever else is wrong
        row(e, "null handle", {"h": None}, INVALID, NULL_HANDLE)
        row(e, "null handle and null buffers", dict(_all_null(e), h=None), INVALID, NULL_HANDLE)
        # a null buffer with a batch of one ...
        for k in _buffers(e):
            row(e, "null " + k, {k: None}, INVALID, NULL_BUFFER)
    # ... and the empty batch: LSCQP_OK with every buffer null, no device asked for
    for e, sizes in (("lscqp_generate_lsc_device", ("n_agents", "n_obs")), ("lscqp_generate_constraints_device", ("n_agents", "n_obs")),
                     ("lscqp_generate_constraints_device_ex", ("n_agents",)), ("lscqp_generate_constraints_own_", ("n_agents",)),
                     ("lscqp_generate_lsc_obstacles_device", ("n_agents",)), ("lscqp_shift_traj_device", ("n",)),
                     ("lscqp_shift_traj_partial_device", ("n",)), ("lscqp_select_neighbours_device", ("n_agents",)),
                     ("lscqp_optimize_goal_device", ("n",)), ("lscqp_optimize_goal_fin_device_", ("n",)), ("lscqp_safety_metrics_device", ("n_agents",)),
                     ("lscqp_safety_obstacles_device", ("n_agents",)), ("lscqp_validate_step_device", ("n",)), ("lscqp_construct_sfc_device", ("n",)),
                     ("lscqp_construct_sfc_device_ordered", ("n",))):
        for k in sizes:
            row(e, "%s = 0 with null buffers" % k, dict(_all_null(e), **{k: 0}), OK, None)
    row("lscqp_generate_constraints_device_ex", "n_obs = 0 with null buffers", dict(_all_null("lscqp_generate_constraints_device_ex"), n_obs=0), OK, None)
    row("lscqp_generate_constraints_own_", "n_obs = 0 with null buffers", dict(_all_null("lscqp_generate_constraints_own_"), n_obs=0), OK, None)
    row("lscqp_generate_lsc_obstacles_device", "n_dyn = 0 with null buffers", dict(_all_null("lscqp_generate_lsc_obstacles_device"), n_dyn=0), OK, None)

    # the generators
    for k in ("n_agents", "n_obs", "first_agent"):
        row("lscqp_generate_lsc_device", k + " < 0", {k: -1}, INVALID, NEGATIVE)
        for e in gens:
            row(e, k + " < 0", {k: -1}, INVALID, NEGATIVE)
    row("lscqp_generate_lsc_device", "negative size and null buffers", dict(_all_null("lscqp_generate_lsc_device"), n_agents=-1), INVALID, NEGATIVE)
    for e in gens:
        for m in (-1, 3):
            row(e, "mode %d" % m, {"mode": m}, INVALID, GEN_MODE)
        row(e, "bad mode and a negative size", {"mode": 3, "n_agents": -1}, INVALID, GEN_MODE)
        row(e, "bad mode and an empty batch", dict(_all_null(e), mode=7, n_agents=0), INVALID, GEN_MODE)
        row(e, "negative size and null buffers", dict(_all_null(e), first_agent=-2), INVALID, NEGATIVE)
    for e in gens[1:]:
        row(e, "slot0 < 0", {"slot0": -1}, INVALID, SLOTS)
        row(e, "n_obs_total < slot0 + n_obs", {"n_obs_total": 4}, INVALID, SLOTS)
        row(e, "slots and a bad mode", {"n_obs_total": 4, "mode": 3}, INVALID, SLOTS)
        row(e, "slots and a negative size", {"slot0": -1, "n_agents": -1}, INVALID, SLOTS)
    e = "lscqp_generate_lsc_obstacles_device"
    row(e, "null param", {"param": None}, INVALID, NULL_HANDLE)
    for k in ("n_agents", "n_dyn", "first_agent", "slot0"):
        row(e, k + " < 0", {k: -1}, INVALID, DYN_SLOTS)
    row(e, "n_obs_total < slot0 + n_dyn", {"n_obs_total": 4}, INVALID, DYN_SLOTS)
    row(e, "slots and null buffers", dict(_all_null(e), n_obs_total=4), INVALID, DYN_SLOTS)
    row(e, "slots and an empty batch", {"n_obs_total": 4, "n_agents": 0}, INVALID, DYN_SLOTS)

    # the shifts
    for e in ("lscqp_shift_traj_device", "lscqp_shift_traj_partial_device"):
        row(e, "n < 0", {"n": -1}, INVALID, NEGATIVE)
        row(e, "n < 0 and null buffers", dict(_all_null(e), n=-1), INVALID, NEGATIVE)
    e = "lscqp_shift_traj_device"
    for v in (-1, 2):
        row(e, "shift_segments %d" % v, {"shift_segments": v}, INVALID, SHIFT)
    row(e, "n < 0 and shift_segments 2", {"n": -1, "shift_segments": 2}, INVALID, NEGATIVE)
    row(e, "shift_segments 2 and an empty batch", dict(_all_null(e), n=0, shift_segments=2), INVALID, SHIFT)
    e = "lscqp_shift_traj_partial_device"
    for v in (0.0, 1.0, -0.25, 1.5, NAN):
        row(e, "fraction %r" % v, {"fraction": v}, INVALID, FRACTION)
    row(e, "n < 0 and fraction 1", {"n": -1, "fraction": 1.0}, INVALID, NEGATIVE)
    row(e, "fraction 0 and an empty batch", dict(_all_null(e), n=0, fraction=0.0), INVALID, FRACTION)

    # neighbours and safety: local block [first_agent, first_agent + n_agents) of n_total agents
    for e, extra in (("lscqp_select_neighbours_device", ("n_obs",)), ("lscqp_safety_metrics_device", ("n_samples",)),
                     ("lscqp_safety_obstacles_device", ("n_samples", "n_obstacles"))):
        for k in ("n_agents", "first_agent") + extra:
            row(e, k + " < 0", {k: -1}, INVALID, INCONSISTENT)
        row(e, "n_total < first_agent + n_agents", {"n_total": 2}, INVALID, INCONSISTENT)
        row(e, "inconsistent sizes and null buffers", dict(_all_null(e), n_total=2), INVALID, INCONSISTENT)
    # a partition: host offsets [0, 4, 10]
    for e, size in (("lscqp_select_neighbours_missions_device", "n_obs"), ("lscqp_safety_metrics_missions_device", "n_samples")):
        row(e, "n_total < 0", {"n_total": -1}, INVALID, INCONSISTENT)
        row(e, size + " < 0", {size: -1}, INVALID, INCONSISTENT)
        row(e, "negative size and no partition", {size: -1, "n_missions": 0, "mission_offsets": None}, INVALID, INCONSISTENT)
        row(e, "n_missions = 0", {"n_missions": 0}, INVALID, PART_NEEDS)
        row(e, "no offset list", {"mission_offsets": None}, INVALID, PART_NEEDS)
        row(e, "offsets start at 1", {"mission_offsets": "off_from_1"}, INVALID, PART_FIRST)
        row(e, "an empty mission", {"mission_offsets": "off_empty", "n_missions": 3}, INVALID, PART_ORDER)
        row(e, "offsets end short of n_total", {"n_total": 11}, INVALID, PART_LAST)
        row(e, "offsets of another mission count", {"n_missions": 1}, INVALID, PART_LAST)
        row(e, "bad partition and null buffers", dict(_all_null(e), n_total=11), INVALID, PART_LAST)

    # the goal LP, the step validation
    for e in ("lscqp_optimize_goal_device", "lscqp_optimize_goal_fin_device_"):
        row(e, "n < 0", {"n": -1}, INVALID, NEGATIVE)
        row(e, "n < 0 and null buffers", dict(_all_null(e), n=-1), INVALID, NEGATIVE)
    e = "lscqp_validate_step_device"
    row(e, "n < 0", {"n": -1}, INVALID, TIME)
    row(e, "time_step < 0", {"time_step": -0.1}, INVALID, TIME)
    row(e, "time_step nan", {"time_step": NAN}, INVALID, TIME)
    row(e, "negative time and null buffers", dict(_all_null(e), time_step=-0.1), INVALID, TIME)
    row(e, "negative time and an empty batch", {"time_step": -0.1, "n": 0}, INVALID, TIME)

    # corridors
    for e in ("lscqp_construct_sfc_device", "lscqp_construct_sfc_device_ordered"):
        row(e, "null map", {"mp": None}, INVALID, NULL_HANDLE)
        for m in (-1, 3):
            row(e, "mode %d" % m, {"mode": m}, INVALID, SFC_MODE)
        row(e, "n < 0", {"n": -1}, INVALID, NEGATIVE)
        row(e, "bad mode and n < 0", {"mode": 3, "n": -1}, INVALID, SFC_MODE)
        row(e, "bad mode and an empty batch", dict(_all_null(e), mode=3, n=0), INVALID, SFC_MODE)
        row(e, "n < 0 and null buffers", dict(_all_null(e), n=-1), INVALID, NEGATIVE)
        row(e, "null map and a bad mode", {"mp": None, "mode": 3}, INVALID, NULL_HANDLE)
    return T


TABLE = _rows()
# Valid arguments: without a device the fixed text, and the buffers that may be NULL are not asked for
VALID = [(e, {}) for e in GOOD] + [
    ("lscqp_select_neighbours_device", {"n_obs": 0, "d_neighbours_out": None}),
    ("lscqp_select_neighbours_missions_device", {"n_obs": 0, "d_neighbours_out": None}),
    ("lscqp_safety_obstacles_device", {"n_obstacles": 0, "d_obstacles": None}),
    ("lscqp_optimize_goal_device", {"h": "h_nosfc", "d_sfc": None}),
    ("lscqp_optimize_goal_fin_device_", {"h": "h_nosfc", "d_sfc": None}),
    ("lscqp_validate_step_device", {"h": "h_nosfc", "d_sfc": None}),
]


@pytest.fixture(scope="module")
def world(api):
    L = api.lib()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    # the one entry of the table that api.lib() has no prototype for (library-internal, csrc/lscqp_internal.hpp)
    L.lscqp_generate_constraints_own_.restype = C.c_int
    L.lscqp_generate_constraints_own_.argtypes = [vp, i32, i64, i32, i64] + [vp] * 7 + [i32, i32, vp]
    solvers = [api.Solver(api.make_desc(M=5, dim=3)), api.Solver(api.make_desc(M=5, dim=3, use_sfc=False)),
               api.Solver(api.make_desc(M=5, dim=3, row_format=api.ROWS_F32))]
    keep = dict(room=(C.c_double * 512)(), map_room=(C.c_double * 512)(), param=api.ObstacleParam(), off=(C.c_int64 * 3)(0, 4, 10),
                off_from_1=(C.c_int64 * 3)(1, 4, 10), off_empty=(C.c_int64 * 4)(0, 4, 4, 10))
    w = dict(L=L, keep=keep, solvers=solvers, h=solvers[0]._h, h_nosfc=solvers[1]._h, h_f32=solvers[2]._h, p=C.cast(keep["room"], vp),
             mp=C.cast(keep["map_room"], vp), param=C.cast(C.pointer(keep["param"]), vp))
    for k in ("off", "off_from_1", "off_empty"):
        w[k] = C.cast(keep[k], vp)
    yield w
    for s in solvers:
        s.close()


def _run(world, entry, change):
    args = dict(GOOD[entry])
    args.update(change)
    vals = [world[v] if isinstance(v, str) else v for v in args.values()]
    return getattr(world["L"], entry)(*vals, None), world["L"].lscqp_last_error().decode()


@pytest.mark.parametrize("entry,what,change,rc,text", TABLE, ids=["%s-%s" % (r[0][6:], r[1].replace(" ", "_")) for r in TABLE])
def test_entry_check(world, entry, what, change, rc, text):
    got, said = _run(world, entry, change)
    assert got == rc, (entry, what, got, said)
    if text is not None:
        assert said == text, (entry, what)


def test_every_entry_has_a_row_that_breaks_two_checks_at_once():
    """... so that the order of the checks is pinned for each of them, not only the checks."""
    for e in GOOD:
        assert any(r[0] == e and len(r[2]) >= 2 and r[3] != OK for r in TABLE), e


def test_generate_lsc_bytes(world):
    """lscqp_generate_lsc_bytes: -1 for a null handle; rows written + control points, radius, downwash + neighbour ids, goal."""
    L = world["L"]
    assert L.lscqp_generate_lsc_bytes(None, 4, 8, 10) == -1
    assert L.lscqp_generate_lsc_bytes(world["h"], 4, 8, 10) == 38304    # 4 * 8 * 30 * 32 + 10 * (30 * 24 + 16) + 4 * (8 * 4 + 24)
    assert L.lscqp_generate_lsc_bytes(world["h_f32"], 4, 8, 10) == 22944  # 16-byte rows
    assert L.lscqp_generate_lsc_bytes(world["h"], 0, 0, 0) == 0


def test_valid_arguments_without_a_device(world):
    """There is no CPU fallback: with every argument in order each entry answers LSCQP_ERR_NO_DEVICE with the one fixed text."""
    n = C.c_int(0)
    if world["L"].hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a device is present; the loud-failure path is for hosts without one")
    for entry, change in VALID:
        got, said = _run(world, entry, change)
        assert (got, said) == (NO_DEVICE, NO_DEVICE_TEXT), (entry, change)
