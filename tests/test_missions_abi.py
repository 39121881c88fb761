"""CPU tests of the mission partition (include/lscqp.h, "many missions over one map"): the new names are declared, exported and wrapped,
the sizes the partition had to leave alone are where they were, the new device entry points refuse a bad partition before they touch the
device, and the per-mission restatement (tests/mission_cases.py) agrees with the single-mission one and keeps missions apart."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

from tests import grid_reference as R
from tests import mission_cases as MC
from tests import waypoint_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lscqp.h")
NEW = ["lscqp_plan_set_missions", "lscqp_plan_missions", "lscqp_plan_mission_status", "lscqp_select_neighbours_missions_device",
       "lscqp_safety_metrics_missions_device", "lscqp_grid_fields_missions_device", "lscqp_waypoints_missions_device", "lscqp_grid_mission_status"]


def test_new_names_are_declared_exported_and_wrapped(api):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = api.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, txt), name
        assert name in api.EXPORTED_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    for cls, meth in ((api.Plan, "set_missions"), (api.Plan, "missions"), (api.Plan, "mission_status"), (api.Grid, "fields_missions"),
                      (api.Grid, "waypoints_missions"), (api.Grid, "mission_status"), (api.Solver, "select_neighbours_missions_device"),
                      (api.Solver, "safety_metrics_missions_device")):
        assert callable(getattr(cls, meth)), meth
    import inspect

    assert "mission_offsets" in inspect.signature(api.Plan.__init__).parameters


def test_plan_desc_and_buffer_count_did_not_move(api):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lscqp.h"\nint main(){printf("%zu %d %zu %zu\\n", sizeof(lscqp_plan_desc),' \
          ' LSCQP_PLAN_BUF_COUNT, offsetof(lscqp_plan_desc, waypoint_mode), offsetof(lscqp_plan_desc, reset_threshold));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        size, count, o_mode, o_thr = map(int, subprocess.check_output([os.path.join(d, "s")]).decode().split())
    assert (size, count) == (96, 19)
    assert C.sizeof(api.PlanDesc) == 96 and api.PlanDesc.waypoint_mode.offset == o_mode and api.PlanDesc.reset_threshold.offset == o_thr


def test_device_entry_points_refuse_a_bad_partition_before_the_device(api):
    """Every check below returns before a device call: the same answers with and without a GPU.  (The grid twins need a grid, which needs a
    device: their NULL-grid check and the shared offset check are what a GPU-less host can see; tests/test_missions_gpu.py has the rest.)"""
    L = api.lib()
    s = api.Solver(api.make_desc(M=10, dim=2))
    h = s._h
    one = (C.c_double * 64)()
    p = C.cast(one, C.c_void_p)

    def off(*v):
        a = (C.c_int64 * len(v))(*v)
        return C.cast(a, C.c_void_p), a

    good, _g = off(0, 4, 10)
    cases = {"non-monotonic": off(0, 6, 4, 10), "empty mission": off(0, 4, 4, 10), "does not start at 0": off(1, 4, 10),
             "does not end at n_total": off(0, 4, 9), "ends beyond n_total": off(0, 4, 11)}
    for what, (bad, _keep) in cases.items():
        K = len(_keep) - 1
        assert L.lscqp_select_neighbours_missions_device(h, 10, K, bad, p, 4, 3.0, p, p, p, None) == api.ERR_INVALID_ARGUMENT, what
        assert b"mission_offsets" in L.lscqp_last_error(), what
        assert L.lscqp_safety_metrics_missions_device(h, 10, K, bad, p, 2, 0.1, 1.0, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT, what
        assert b"mission_offsets" in L.lscqp_last_error(), what
    for K, o in ((0, good), (2, None)):
        assert L.lscqp_select_neighbours_missions_device(h, 10, K, o, p, 4, 3.0, p, p, p, None) == api.ERR_INVALID_ARGUMENT
        assert L.lscqp_safety_metrics_missions_device(h, 10, K, o, p, 2, 0.1, 1.0, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    # a good partition: the other arguments are still checked
    assert L.lscqp_select_neighbours_missions_device(None, 10, 2, good, p, 4, 3.0, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_select_neighbours_missions_device(h, 10, 2, good, None, 4, 3.0, p, p, p, None) == api.ERR_INVALID_ARGUMENT  # no device copy
    assert L.lscqp_select_neighbours_missions_device(h, 10, 2, good, p, -1, 3.0, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_safety_metrics_missions_device(h, 10, 2, good, p, 2, 0.1, 1.0, p, None, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_safety_metrics_missions_device(h, 10, 2, good, p, -2, 0.1, 1.0, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    # the grid twins and the plan calls without their object
    assert L.lscqp_grid_fields_missions_device(None, 10, 2, good, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_waypoints_missions_device(None, 3.0, 10, 2, 10, 2, good, p, p, p, p, p, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_grid_mission_status(None, 2, p) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_plan_set_missions(None, 2, good) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_plan_missions(None, p, p) == api.ERR_INVALID_ARGUMENT and L.lscqp_plan_mission_status(None, p) == api.ERR_INVALID_ARGUMENT
    import torch

    if not torch.cuda.is_available():
        assert L.lscqp_select_neighbours_missions_device(h, 10, 2, good, p, 4, 3.0, p, p, p, None) == api.ERR_NO_DEVICE
        assert L.lscqp_safety_metrics_missions_device(h, 10, 2, good, p, 2, 0.1, 1.0, p, p, p, p, p, None) == api.ERR_NO_DEVICE
        assert b"no CPU fallback" in L.lscqp_last_error()
    s.close()


def test_restatement_with_one_mission_is_the_single_mission_restatement(oracle):
    world, off, starts, goals = MC.forest_missions(1, n=10, side=20.0, n_boxes=60, seed=5)
    G = WC.reference_grid(oracle, world)
    F1, d1 = R.mission_fields(G, list(starts), list(goals))
    free1 = G.free.copy()
    F, d, free = MC.mission_fields(G, off, starts, goals)
    assert np.array_equal(F, F1) and np.array_equal(d, d1) and np.array_equal(free[0], free1)
    w = dict(world, starts=[list(p) for p in starts])
    for rng in (-1, 0.0, 3.0):
        G.free = free1
        single = WC.seeded_states(G, w, F1, d1, 4, rng, seed=9)
        multi = MC.seeded_states(G, free, off, world, starts, F, d, 4, rng, seed=9)
        for s1, sK in zip(single, multi):
            assert all(np.array_equal(s1[key], sK[key]) for key in s1)
            G.free = free1
            a = R.waypoint_step(G, rng, s1["positions"], list(s1["plans"]), s1["current_goals"], s1["waypoints"], F1, d1)
            b = MC.waypoint_step(G, free, off, rng, sK["positions"], sK["plans"], sK["current_goals"], sK["waypoints"], F, d)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_mission_does_not_change_when_others_are_added_around_it(oracle):
    K, n = 3, 10
    world, off, starts, goals = MC.forest_missions(K, n=n, side=20.0, n_boxes=60, seed=5)
    G = WC.reference_grid(oracle, world)
    F, d, free = MC.mission_fields(G, off, starts, goals)
    states = MC.seeded_states(G, free, off, world, starts, F, d, 3, 3.0, seed=21)
    seen_shared = 0
    for k, sl in enumerate(MC.slices(off)):
        _, off1, s1, g1 = MC.forest_missions(k + 1, n=n, side=20.0, n_boxes=60, seed=5)
        s1, g1 = s1[sl], g1[sl]  # mission k, drawn again on its own
        assert np.array_equal(s1, starts[sl]) and np.array_equal(g1, goals[sl])
        Fk, dk, freek = MC.mission_fields(G, [0, n], s1, g1)
        assert np.array_equal(Fk, F[sl]) and np.array_equal(dk, d[sl]) and np.array_equal(freek[0], free[k])
        for s in states:
            alone = MC.waypoint_step(G, freek, [0, n], 3.0, s["positions"][sl], s["plans"][sl], s["current_goals"][sl], s["waypoints"][sl], Fk, dk)
            among = MC.waypoint_step(G, free, off, 3.0, s["positions"], s["plans"], s["current_goals"], s["waypoints"], F, d)
            assert np.array_equal(alone[0] + off[k], among[0][sl])
            assert all(np.array_equal(x, y[sl]) for x, y in zip(alone[1:], among[1:]))
        # the missions do overlap in space: agents of other missions stand within range of this one's (one swarm would group them)
        others = np.r_[0:sl.start, sl.stop:K * n]
        seen_shared += int((np.abs(states[0]["positions"][sl][:, None, :] - states[0]["positions"][others][None]).max(axis=2) < 3.0).sum())
    assert seen_shared > 0
