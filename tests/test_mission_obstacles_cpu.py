"""A mission's own obstacles without a device (include/lscqp.h, "a mission's own obstacles"): the ABI, and every check the three device
entries make before they touch the device -- the offset list above all.  The refusals of lscqp_plan_set_mission_obstacles need a plan, and a
plan needs a device: tests/test_mission_obstacles_plan_gpu.py holds them."""
import ctypes as C
import os
import re

import numpy as np

from tests import mission_obstacles_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lscqp.h")
NEW = ["lscqp_obstacles_advance_missions_device", "lscqp_obstacles_drive_missions_device", "lscqp_safety_obstacles_ids_device",
       "lscqp_plan_set_mission_obstacles"]


def _solver(api):
    return api.Solver(api.make_desc(M=5, dim=3))


def test_every_entry_is_declared_once_exported_and_resolves(api):
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = api.lib()
    want_args = dict(zip(NEW, (10, 16, 16, 5)))
    for name in NEW:
        assert len(re.findall(r"\b%s\s*\(" % name, txt)) == 1, name
        assert api.EXPORTED_SYMBOLS.count(name) == 1 and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == want_args[name], name
    for owner, meth in ((api.Plan, "set_mission_obstacles"), (api.Solver, "obstacles_advance_missions_device"),
                        (api.Solver, "obstacles_drive_missions_device"), (api.Solver, "safety_obstacles_ids_device")):
        assert callable(getattr(owner, meth))
    # the header no longer says that a partition can only share its obstacles, and says what the buffers hold with a table per mission
    assert "A mission partition shares the obstacles like the map" not in " ".join(raw.split())
    assert "int32[n_missions]" in raw and "a mission's own obstacles" in raw


def test_the_offset_list_is_checked_before_the_device_is_touched(api):
    """Not from 0, decreasing, last != total: LSCQP_ERR_INVALID_ARGUMENT each with its cause; one mission over lscqp_max_obstacles:
    LSCQP_ERR_UNSUPPORTED -- while a TOTAL above it is no objection.  Both entries that take the list make the same check."""
    sol = _solver(api)
    L, h = api.lib(), sol._h
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    last = lambda: L.lscqp_last_error().decode()  # noqa: E731
    cap = sol.max_obstacles()
    assert cap >= 65  # (the kernel tests fly missions of 65)

    def advance(off, total, models=p):
        o = np.ascontiguousarray(off, np.int32)
        return L.lscqp_obstacles_advance_missions_device(h, models, len(o) - 1, o.ctypes.data_as(C.c_void_p), p, total, 0.2, p, p, None)

    def drive(off, total):
        o = np.ascontiguousarray(off, np.int32)
        return L.lscqp_obstacles_drive_missions_device(h, p, p, len(o) - 1, o.ctypes.data_as(C.c_void_p), p, total, p, 1, p, 1, p, 0.2, p, p, None)

    import torch

    for entry in (advance, drive):
        assert entry([1, 2, 3], 3) == api.ERR_INVALID_ARGUMENT and last() == "obstacle_offsets[0] must be 0"
        assert entry([0, 2, 1], 1) == api.ERR_INVALID_ARGUMENT and last() == "obstacle_offsets must not decrease"
        assert entry([0, 1, 3], 4) == api.ERR_INVALID_ARGUMENT and last() == "obstacle_offsets[n_missions] must be n_dyn_total"
        assert entry([0, 1, cap + 2], cap + 2) == api.ERR_UNSUPPORTED and "a mission's obstacle count exceeds" in last() and "lscqp_max_obstacles" in last()
        if not torch.cuda.is_available():  # every mission at the cap, the total K times it: accepted as far as the device
            assert entry([0, cap, 2 * cap, 3 * cap], 3 * cap) == api.ERR_NO_DEVICE and last() == "no HIP device: lscqp has no CPU fallback"
    sol.close()


def test_sizes_null_buffers_and_the_empty_batch(api):
    sol = _solver(api)
    L, h = api.lib(), sol._h
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    last = lambda: L.lscqp_last_error().decode()  # noqa: E731
    off = np.array([0, 1, 1, 2], np.int32)
    o = off.ctypes.data_as(C.c_void_p)
    adv, drv, saf = L.lscqp_obstacles_advance_missions_device, L.lscqp_obstacles_drive_missions_device, L.lscqp_safety_obstacles_ids_device
    # --- the advance
    assert adv(None, p, 3, o, p, 2, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and last() == "null handle"
    for K, total, ts in ((-1, 2, 0.2), (3, -1, 0.2), (3, 2, 0.0), (3, 2, float("nan")), (3, 2, float("inf"))):
        assert adv(h, p, K, o, p, total, ts, p, p, None) == api.ERR_INVALID_ARGUMENT and "inconsistent sizes" in last()
    assert adv(h, None, 0, None, None, 0, 0.2, None, None, None) == api.OK  # the empty batch: no device either
    assert adv(h, p, 3, None, p, 2, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and "needs n_missions >= 1 and its obstacle_offsets" in last()
    for hole in (1, 4, 7, 8):  # models, the device's offsets, the clocks, the table
        args = [h, p, 3, o, p, 2, 0.2, p, p, None]
        args[hole] = None
        assert adv(*args) == api.ERR_INVALID_ARGUMENT and last() == "null buffer", hole
    # --- the drive
    assert drv(None, p, p, 3, o, p, 2, p, 1, p, 1, p, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and last() == "null handle"
    for K, total, nh, nt, ts in ((-1, 2, 0, 0, 0.2), (3, -1, 0, 0, 0.2), (3, 2, -1, 0, 0.2), (3, 2, 0, -1, 0.2), (3, 2, 0, 0, -0.2)):
        assert drv(h, p, p, K, o, p, total, p, nh, p, nt, p, ts, p, p, None) == api.ERR_INVALID_ARGUMENT and "inconsistent sizes" in last()
    assert drv(h, None, None, 0, None, None, 0, None, 0, None, 0, None, 0.2, None, None, None) == api.OK  # the empty batch
    zero = np.zeros(4, np.int32)  # missions none of which owns an obstacle: nothing to move, no device
    assert drv(h, None, None, 3, zero.ctypes.data_as(C.c_void_p), None, 0, None, 0, None, 0, None, 0.2, None, None, None) == api.OK
    for hole in (1, 2, 5, 11, 13, 14):  # models, drives, the device's offsets, checkpoints, clocks, table
        args = [h, p, p, 3, o, p, 2, p, 1, p, 1, p, 0.2, p, p, None]
        args[hole] = None
        assert drv(*args) == api.ERR_INVALID_ARGUMENT and last() == "null buffer", hole
    assert drv(h, p, p, 3, o, p, 2, None, 1, p, 1, p, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"  # an announced history
    assert drv(h, p, p, 3, o, p, 2, p, 1, None, 1, p, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"  # an announced state
    # --- the safety figures by ids
    ok = [h, 4, 0, 4, 2, 0.1, 1.0, p, p, p, 3, p, 5, p, p, None]
    assert saf(*([None] + ok[1:])) == api.ERR_INVALID_ARGUMENT and last() == "null handle"
    for at, bad in ((1, -1), (2, -1), (4, -1), (10, -1), (12, -1), (3, 3)):  # n_agents, first_agent, n_samples, n_slots, n_obstacles, n_total
        args = list(ok)
        args[at] = bad
        assert saf(*args) == api.ERR_INVALID_ARGUMENT and last() == "inconsistent sizes", at
    args = list(ok)
    args[1] = 0
    assert saf(*[a if i not in (7, 8, 9, 11, 13, 14) else None for i, a in enumerate(args)]) == api.OK  # no agent: no device either
    for hole in (7, 8, 9, 11, 13, 14):  # plans, radii, downwash, ids, table, out
        args = list(ok)
        args[hole] = None
        assert saf(*args) == api.ERR_INVALID_ARGUMENT and last() == "null buffer", hole
    assert L.lscqp_plan_set_mission_obstacles(None, p, 1, o, p) == api.ERR_INVALID_ARGUMENT and last() == "null plan"
    sol.close()


def test_the_cases_cover_what_the_kernel_tests_say_they_cover(api):
    counts = {c for s in MC.SHAPES for c in s}
    assert counts == {0, 1, 63, 64, 65} and {len(s) for s in MC.SHAPES} == {1, 2, 3} and len(set(MC.CLOCKS)) == 3
    models = api.obstacle_model_prepare(api.obstacle_models(MC.advance_specs(8, 1)))
    assert set(models["kind"].tolist()) == {api.OBSTACLE_HELD, api.OBSTACLE_STRAIGHT, api.OBSTACLE_PATROL, api.OBSTACLE_SPIN}
    m, d, hist = MC.drive_tables(api, (5, 0, 10), 6)
    api.obstacle_drive_check(m, d, len(hist), 6)
    assert set(d["kind"].tolist()) == {api.DRIVE_NONE, api.DRIVE_CHASING, api.DRIVE_GAUSSIAN}
    g = d[d["kind"] == api.DRIVE_GAUSSIAN]
    assert len(g) == 3 and (g["history_first"] == 0).all() and (g["history_len"] == len(hist)).all()  # one slice, shared across missions
    assert (d["target_agent"][d["kind"] == api.DRIVE_CHASING] >= 0).any() and (d["target_agent"][d["kind"] == api.DRIVE_CHASING] < 0).any()
    m, d, off = MC.neighbours_across_missions(api)
    gap = np.linalg.norm(np.float32(m["start"][0]) - np.float32(m["start"][2]))
    assert off.tolist() == [0, 2, 4] and 1e-5 < gap < 2 * (m["radius"][0] + m["radius"][2])  # inside Q*, in different missions
    for own in ((0, 1), (2, 3)):
        assert np.linalg.norm(m["start"][own[0]] - m["start"][own[1]]) > 2 * (m["radius"][own[0]] + m["radius"][own[1]])
    rows = MC.ID_ROWS
    assert (rows[:, 0] == -1).any() and (rows[:, -1] == -1).any() and (rows == MC.REAL).any() and (rows == -1).all(1).any()
    tie = rows[2].tolist()
    assert tie.index(MC.TWIN_B) < tie.index(MC.TWIN_A) and MC.TWIN_B > MC.TWIN_A  # the lower slot holds the higher table index
    c = MC.safety_case(api, 65)
    assert c["table"][MC.TWIN_A].tobytes() == c["table"][MC.TWIN_B].tobytes() and c["table"]["type"][MC.REAL] == api.OBSTACLE_REAL
