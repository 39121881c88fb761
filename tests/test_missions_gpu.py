"""Many missions over one map on the device (include/lscqp.h, "many missions over one map"): the mission-aware entry points against the
per-mission restatement (tests/mission_cases.py) and against the single-mission entry points run on each slice, and plans with a mission
partition against plans without one.  Everything compared is integers, exact grid points or the bits of a buffer: exact equality throughout."""
import os

import numpy as np
import pytest

from tests import grid_reference as R
from tests import mission_cases as MC
from tests import waypoint_cases as WC
from tests import waypoint_device as WD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _device_step(torch, grid, off, rng, s, d_field, d_init_d):
    return WD.decision_step(torch, grid, rng, s, d_field, d_init_d, off=off)


def _compare_rollouts(api, torch, grid, G, world, off, starts, goals, ranges, steps, seed):
    F, init_d, free = MC.mission_fields(G, off, starts, goals)
    d_field, d_init_d = grid.fields_missions(off, WD.dev(torch, starts, np.float64), WD.dev(torch, goals, np.float64))
    torch.cuda.synchronize()
    assert np.array_equal(d_field.cpu().numpy(), F)
    assert np.array_equal(d_init_d.cpu().numpy(), init_d)
    n_updated, n_groups = 0, set()
    for rng in ranges:
        for s in MC.seeded_states(G, free, off, world, starts, F, init_d, steps, rng, seed):
            label, desired, updated, new = MC.waypoint_step(G, free, off, rng, s["positions"], s["plans"], s["current_goals"], s["waypoints"], F, init_d)
            g, d, u, w = _device_step(torch, grid, off, rng, s, d_field, d_init_d)
            assert np.array_equal(d, desired), (rng, np.nonzero(d != desired))
            assert np.array_equal(g, label), (rng, np.nonzero(g != label))  # (= offset + the slice's own least id)
            assert np.array_equal(u, updated), (rng, np.nonzero(u != updated))
            assert np.array_equal(w, new), rng
            for k, sl in enumerate(MC.slices(off)):  # a group never spans missions
                assert off[k] <= g[sl].min() and g[sl].max() < off[k + 1]
            n_updated += int(updated.sum())
            n_groups.add(len(set(label.tolist())))
    return n_updated, n_groups, dict(F=F, init_d=init_d, free=free, d_field=d_field, d_init_d=d_init_d)


_FOREST = {}


def _forest_grid(oracle, world):
    """The restatement's grid of the 40 m forest (node by node in Python: made once per session)."""
    if "G" not in _FOREST:
        _FOREST["G"] = WC.reference_grid(oracle, world)
    return _FOREST["G"]


@pytest.mark.parametrize("K", [1, 3, 25])
def test_waypoint_twins_equal_the_per_mission_restatement_lds_tables(api, oracle, torch_cuda, K):
    """The 40 m forest (81 x 81 nodes: node tables in LDS), K seeded ten-agent missions, ranges -1 (one group per mission), 0 (every agent alone)
    and 3 m: fields, init_d, desired nodes, waypoints, updated flags and groups."""
    import torch

    world, off, starts, goals = MC.forest_missions(K, n=10, side=40.0, n_boxes=300, seed=0)
    wmap, grid = WD.device_grid(api, world)
    G = _forest_grid(oracle, world)
    assert grid.dims.tolist() == G.dims and np.array_equal(grid.download().astype(bool), G.occ)
    assert 2 * G.W * G.H * 4 <= 60 * 1024
    n_updated, n_groups, _ = _compare_rollouts(api, torch, grid, G, world, off, starts, goals, (-1, 0.0, 3.0), 3, seed=17)
    assert n_updated > 5 * K and K in n_groups and 10 * K in n_groups, (n_updated, n_groups)
    grid.close()
    wmap.close()


def test_waypoint_twins_equal_the_per_mission_restatement_hbm_tables(api, oracle, torch_cuda):
    """walled_world(400): 160 000 nodes, fields relaxed in HBM and the node tables of each mission in its slab of the HBM buffer.  Mission 0
    is the world's own three agents.  Mission 1 -- the one whose slab does not start at the buffer -- has an agent that crosses the world
    and two that meet head-on in the open: A (agent 3) wants to go right through B (agent 4), B wants to go left through A and has the
    priority (init_d 5 against 4), so B takes A's node and A, by priority inheritance, has to back off AWAY from its goal.  Ranges -1, 0
    and 3 m.  Occupancy from the device (its rule is tested on the smaller worlds)."""
    import torch

    w = WC.walled_world(400)
    wmap, grid = WD.device_grid(api, w)
    assert grid.dims.tolist() == [400, 400, 1]
    G = R.Grid(w["world_min"], w["world_max"], w["z_2d"], 0.5, w["radius"], occ=grid.download().astype(bool))
    A_start, A_goal, B_start, B_goal = [10.0, 5.0, 0.6], [12.0, 5.0, 0.6], [10.5, 5.0, 0.6], [8.0, 5.0, 0.6]
    starts = np.array(w["starts"] + [A_start, B_start, w["goals"][0]], float)
    goals = np.array(w["goals"] + [A_goal, B_goal, w["starts"][0]], float)
    off = np.array([0, 3, 6])
    n_updated, n_groups, c = _compare_rollouts(api, torch, grid, G, w, off, starts, goals, (-1, 0.0, 3.0), 2, seed=4)
    assert n_updated > 0 and {2, 6} <= n_groups, (n_updated, n_groups)  # (range -1: one group per mission; range 0: every agent alone)
    assert c["init_d"][3] == 4 and c["init_d"][4] == 5
    # the head-on pair at its start, one group per mission: the walk of mission 1 runs in ITS slab, with a conflict in it
    s = dict(positions=starts, plans=None, current_goals=starts, waypoints=starts)
    g, d, u, way = _device_step(torch, grid, off, -1, s, c["d_field"], c["d_init_d"])
    ref = MC.waypoint_step(G, c["free"], off, -1, starts, None, starts, starts, c["F"], c["init_d"])
    assert all(np.array_equal(x, y) for x, y in zip((g, d, u, way), ref))
    assert g.tolist() == [0, 0, 0, 3, 3, 3]
    (ax, ay), (bx, by) = G.node(A_start), G.node(B_start)
    assert d[4] == ay * G.W + ax                      # B takes A's node ...
    assert d[3] not in (ay * G.W + ax, by * G.W + bx)  # ... A neither stays nor swaps:
    assert c["F"][3].reshape(-1)[d[3]] == 5            # it steps back, one step further from its goal than it was
    # the same decision again: the slabs were left empty by the walk before
    g2, d2, _, _ = _device_step(torch, grid, off, -1, s, c["d_field"], c["d_init_d"])
    assert np.array_equal(g2, g) and np.array_equal(d2, d)
    grid.close()
    wmap.close()


def test_start_and_goal_nodes_are_cleared_in_their_own_mission_only(api, oracle, torch_cuda):
    """Mission A's goal is an OCCUPIED node G in a wall; B's start is above it and B's goal below it.  Were G free in B's graph, B would reach
    its goal in 2 steps through G.  It is free in A's graph only: A's field reaches it, B's field goes round the wall (6 steps) and B's
    candidate below its start does not exist."""
    import torch

    rows = [".....",
            "####.",
            "....."]
    world = WC.toy_world(rows)
    Wd = len(rows[0])
    A_start, A_goal, B_start, B_goal = WC.P(0, 0), WC.P(2, 1), WC.P(2, 0), WC.P(2, 2)
    starts, goals = np.array([A_start, B_start], float), np.array([A_goal, B_goal], float)
    off = np.array([0, 1, 2])
    wmap, grid = WD.device_grid(api, world)
    assert np.array_equal(grid.download().astype(bool), world["occ"])
    G = WC.reference_grid(oracle, world)
    F, init_d, free = MC.mission_fields(G, off, starts, goals)
    gi, gj = G.node(A_goal)
    assert G.occ[gj, gi] and free[0][gj, gi] and not free[1][gj, gi]
    d_field, d_init_d = grid.fields_missions(off, WD.dev(torch, starts, np.float64), WD.dev(torch, goals, np.float64))
    got, got_d = d_field.cpu().numpy(), d_init_d.cpu().numpy()
    assert np.array_equal(got, F) and np.array_equal(got_d, init_d)
    assert got[0, gj, gi] == 0 and got_d[0] == 3            # A: (0,0) -> (1,0) -> (2,0) -> G
    assert got[1, gj, gi] == api.GRID_UNREACHABLE and got_d[1] == 6  # B: round the wall through (4, 1)
    s = dict(positions=starts, plans=None, current_goals=starts, waypoints=starts)
    g, d, u, w = _device_step(torch, grid, off, -1, s, d_field, d_init_d)
    ref = MC.waypoint_step(G, free, off, -1, starts, None, starts, starts, F, init_d)
    assert all(np.array_equal(x, y) for x, y in zip((g, d, u, w), ref))
    assert d.tolist() == [WC.N(1, 0, Wd), WC.N(3, 0, Wd)] and g.tolist() == [0, 1]  # B steps right, not down into G
    # the same two agents as ONE mission: G is free for both and B goes through it
    f1, d1 = grid.fields(WD.dev(torch, starts, np.float64), WD.dev(torch, goals, np.float64))
    torch.cuda.synchronize()
    assert d1.cpu().numpy().tolist() == [3, 2]
    grid.close()
    wmap.close()


def _positions(rng, off, side):
    n = int(off[-1])
    pos = np.c_[rng.uniform(-side, side, (n, 2)), np.full(n, 0.6)]
    return np.float32(pos).astype(np.float64)


def test_neighbour_twin_equals_the_single_entry_point_on_each_slice(api, torch_cuda):
    """Missions of 7, 33, 1 and 1100 agents in one box: a mission of one, slices that are no multiple of the wavefront, a cut to the n_obs
    nearest, and more than 1024 agents in range (the bisection form).  Ids shifted by the offset, bits equal."""
    import torch

    sol = api.Solver(api.make_desc(M=10, dim=2))
    off = np.array([0, 7, 40, 41, 1141])
    n = int(off[-1])
    pos = _positions(np.random.default_rng(3), off, 6.0)
    d_pos = WD.dev(torch, pos)
    for n_obs, rng in ((8, 3.0), (8, -1.0), (40, 1.5), (0, 3.0)):
        d_nbr = torch.full((n * max(n_obs, 1),), -7, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        sol.select_neighbours_missions_device(off, n_obs, rng, d_pos, d_nbr, d_cnt)
        torch.cuda.synchronize()
        nbr, cnt = d_nbr.cpu().numpy()[:n * n_obs].reshape(n, n_obs), d_cnt.cpu().numpy()
        for k, sl in enumerate(MC.slices(off)):
            nk = sl.stop - sl.start
            s_nbr = torch.full((nk * max(n_obs, 1),), -7, dtype=torch.int32, device="cuda")
            s_cnt = torch.full((nk,), -7, dtype=torch.int32, device="cuda")
            sol.select_neighbours_device(nk, 0, nk, n_obs, rng, WD.dev(torch, pos[sl]), s_nbr, s_cnt)
            torch.cuda.synchronize()
            want = s_nbr.cpu().numpy()[:nk * n_obs].reshape(nk, n_obs)
            want = np.where(want >= 0, want + off[k], want)
            assert np.array_equal(nbr[sl], want), (n_obs, rng, k)
            assert np.array_equal(cnt[sl], s_cnt.cpu().numpy()), (n_obs, rng, k)
        assert cnt[40] == 0 and (n_obs == 0 or (nbr[40] == -1).all())  # the mission of one has nobody
    assert cnt[41:].max() > 8
    sol.close()


def test_safety_twin_equals_the_single_entry_point_on_each_slice(api, torch_cuda):
    import torch

    M, dim = 10, 2
    sol = api.Solver(api.make_desc(M=M, dim=dim))
    off = np.array([0, 7, 40, 41, 300])
    n = int(off[-1])
    rnd = np.random.default_rng(8)
    pos = _positions(rnd, off, 4.0)
    x = pos[:, :2, None, None] + np.cumsum(rnd.uniform(-0.05, 0.12, (n, dim, M, 6)), axis=3)
    x = np.float32(x).astype(np.float64).reshape(n, -1)
    rad, dwv = rnd.choice([0.15, 0.25], n), rnd.choice([2.0, 1.2], n)
    hdr = np.zeros(n, api.HEADER_DTYPE)
    hdr["vmax"], hdr["amax"] = 0.3, 1.0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")  # noqa: E731
    d_out = torch.zeros(n * api.SAFETY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    sol.safety_metrics_missions_device(off, 3, 0.07, WD.dev(torch, x), WD.dev(torch, rad), WD.dev(torch, dwv), up(hdr), d_out, z_2d=0.6)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(api.SAFETY_DTYPE)
    for k, sl in enumerate(MC.slices(off)):
        nk = sl.stop - sl.start
        s_out = torch.zeros(nk * api.SAFETY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        sol.safety_metrics_device(nk, 0, nk, 3, 0.07, WD.dev(torch, x[sl]), WD.dev(torch, rad[sl]), WD.dev(torch, dwv[sl]), up(hdr[sl]), s_out, z_2d=0.6)
        torch.cuda.synchronize()
        want = s_out.cpu().numpy().view(api.SAFETY_DTYPE).copy()
        want["closest_agent"] = np.where(want["closest_agent"] >= 0, want["closest_agent"] + off[k], want["closest_agent"])
        assert got[sl].tobytes() == want.tobytes(), k
    assert got["closest_agent"][40] == -1 and np.isinf(got["safety_ratio"][40])
    assert got["vel_excess_ratio"].max() > 0 and np.isfinite(got["safety_ratio"][:40]).all()
    sol.close()


def _plan(api, sol, wmap, W, N, **kw):
    return api.Plan(sol, wmap, N, 9, WD.agents(api, W["radius"], N), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True,
                    closed_loop=True, z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT, **kw)


def _snapshot(api, plan, n):
    """Every buffer of the plan as (n, bytes per agent) uint8 rows, with the two that hold agent ids turned into ids relative to nothing."""
    out = {}
    for b in range(19):
        a = plan.get(b)
        out[b] = a.copy() if b in (api.PLAN_GROUP, api.PLAN_SAFETY) else np.ascontiguousarray(a).view(np.uint8).reshape(n, -1).copy()
    return out


def _slice_of(api, snap, sl, base):
    """Mission slice of a snapshot, ids made local to the mission."""
    out = {}
    for b, a in snap.items():
        v = a[sl].copy()
        if b == api.PLAN_GROUP:
            v = v - base
        elif b == api.PLAN_SAFETY:
            v["closest_agent"] = np.where(v["closest_agent"] >= 0, v["closest_agent"] - base, v["closest_agent"])
        out[b] = np.ascontiguousarray(v).view(np.uint8).reshape(sl.stop - sl.start, -1)
    return out


def _same(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def _fly(api, torch, plan, n, steps, graph, starts, goals):
    plan.reset(starts, goals)
    trace = []
    for _ in range(steps):
        plan.step(graph=graph)
        torch.cuda.synchronize()
        trace.append(_snapshot(api, plan, n))
    return trace


def test_copies_of_forest10_fly_as_one(api, torch_cuda):
    """25 copies of the forest10 mission literally on top of each other in one plan, closed loop, 79 replans, waypoint_mode 1: every mission's
    slice of every buffer is bit-identical to mission 0's and to a plan of ten agents without a partition; eager and graph runs are
    bit-identical; no walk reaches its bound."""
    import torch

    W = WC.forest10()
    K, n, steps = 25, 10, 79
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    off = np.arange(K + 1) * n
    single = _plan(api, sol, wmap, W, n)
    assert single.missions().tolist() == [0, n]
    single.reset(starts, goals)
    many = {}
    for graph in (False, True):
        many[graph] = _plan(api, sol, wmap, W, K * n, mission_offsets=off)
        assert many[graph].missions().tolist() == off.tolist()
        many[graph].reset(np.tile(starts, (K, 1)), np.tile(goals, (K, 1)))
    moved = 0
    for t in range(steps):  # (the three flights in step: nothing but the last replan's buffers is kept)
        single.step(graph=True)
        for graph in (False, True):
            many[graph].step(graph=graph)
        torch.cuda.synchronize()
        ref = _slice_of(api, _snapshot(api, single, n), slice(0, n), 0)
        eager, replay = _snapshot(api, many[False], K * n), _snapshot(api, many[True], K * n)
        assert not _same(eager, replay), (t, _same(eager, replay))
        for k, sl in enumerate(MC.slices(off)):
            diff = _same(_slice_of(api, replay, sl, int(off[k])), ref)
            assert not diff, (t, k, diff)
        moved += int(ref[api.PLAN_WAYPOINT_UPDATED].view(np.int32).sum())
    assert single.mission_status().tolist() == [0]
    for graph in (False, True):
        assert not many[graph].mission_status().any() and (many[graph].graph_nodes() > 0) == graph
        many[graph].close()
    single.close()
    assert moved > 100
    wmap.close()
    sol.close()


def test_distinct_missions_fly_as_their_own_plans_would(api, torch_cuda):
    """25 distinct seeded ten-agent missions on one 40 m forest, 30 closed-loop replans: one plan with the partition against 25 plans of ten
    agents, every buffer slice bit for bit, statuses included.  250 QPs and 10 QPs both lie inside the launch policy's smallest class on a
    256-CU device (one workgroup per QP, the same kernel form per instance), so the solver gives the same bits either way."""
    import torch

    K, n, steps = 25, 10, 30
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert K * n <= cus, "sized for a device with at least %d compute units (found %d)" % (K * n, cus)
    W, off, starts, goals = MC.forest_missions(K, n=n, side=40.0, n_boxes=300, seed=0)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    plan = _plan(api, sol, wmap, W, K * n, mission_offsets=off)
    got = _fly(api, torch, plan, K * n, steps, True, starts, goals)
    assert not plan.mission_status().any()
    plan.close()
    qp_status = np.concatenate([g[api.PLAN_STATUS].view(np.int32).reshape(-1) for g in got])
    print("distinct missions: QP statuses over the flight:", dict(zip(*np.unique(qp_status, return_counts=True))))
    for k, sl in enumerate(MC.slices(off)):
        one = _plan(api, sol, wmap, W, n)
        want = _fly(api, torch, one, n, steps, True, starts[sl], goals[sl])
        assert one.mission_status().tolist() == [0]
        one.close()
        for t in range(steps):
            mine = _slice_of(api, got[t], sl, int(off[k]))
            diff = _same(mine, _slice_of(api, want[t], slice(0, n), 0))
            assert not diff, (k, t, diff)
    wmap.close()
    sol.close()


def test_refusals_and_the_single_mission_plan(api, torch_cuda):
    import torch

    W = WC.forest10()
    n = 10
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    plan = _plan(api, sol, wmap, W, n)
    for bad in ([0, 6, 4, 10], [0, 4, 4, 10], [1, 4, 10], [0, 4, 9], [0, 4, 11]):
        with pytest.raises(api.LscqpError) as e:
            plan.set_missions(bad)
        assert e.value.code == api.ERR_INVALID_ARGUMENT and "mission_offsets" in str(e.value), bad
        assert plan.missions().tolist() == [0, n]  # (a refused call leaves the plan as it was)
    plan.reset(starts, goals)
    plan.step()  # ... and steppable
    plan.set_missions([0, 4, 10])
    assert plan.missions().tolist() == [0, 4, 10]
    for graph in (False, True):
        with pytest.raises(api.LscqpError) as e:  # no step between set_missions and the reset
            plan.step(graph=graph)
        assert e.value.code == api.ERR_INVALID_ARGUMENT and "lscqp_plan_reset" in str(e.value)
    plan.reset(starts, goals)
    for _ in range(3):
        plan.step(graph=True)
    torch.cuda.synchronize()
    grp = plan.get(api.PLAN_GROUP)
    assert grp[:4].max() < 4 <= grp[4:].min() and plan.mission_status().tolist() == [0, 0]
    nbr_count = plan.get(api.PLAN_IN_RANGE)
    assert nbr_count[:4].max() <= 3 and nbr_count[4:].max() <= 5
    # n_missions = 1 (and None) is the plan without the call, bit for bit
    ref_plan = _plan(api, sol, wmap, W, n)
    ref = _fly(api, torch, ref_plan, n, 12, True, starts, goals)
    nodes = ref_plan.graph_nodes()
    ref_plan.close()
    for offsets in ([0, n], None):
        plan.set_missions(offsets)
        assert plan.missions().tolist() == [0, n]
        with pytest.raises(api.LscqpError):
            plan.step()
        got = _fly(api, torch, plan, n, 12, True, starts, goals)
        assert all(not _same(a, b) for a, b in zip(got, ref)) and plan.graph_nodes() == nodes
        assert plan.mission_status().tolist() == [0]
    plan.close()
    # a sharded plan flies one mission
    shard = api.Plan(sol, wmap, 5, 9, WD.agents(api, W["radius"], n), n_total=n, first_agent=0, constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL,
                     z_2d=W["z_2d"])
    with pytest.raises(api.LscqpError) as e:
        shard.set_missions([0, 4, 10])
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "n_agents == n_total" in str(e.value)
    shard.set_missions(None)
    shard.close()
    # the grid twins: a bad partition, and a decision before the fields of its partition
    grid = api.Grid(wmap, 0.5, W["radius"], W["z_2d"])
    d_s, d_g = WD.dev(torch, starts, np.float64), WD.dev(torch, goals, np.float64)
    with pytest.raises(api.LscqpError) as e:
        grid.fields_missions([0, 6, 4, 10], d_s, d_g)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    d_way = d_s.clone()
    with pytest.raises(api.LscqpError) as e:
        grid.waypoints_missions([0, 4, 10], 3.0, 10, 2, WD.dev(torch, np.zeros((n, 9))), None, d_s, torch.zeros(n, dtype=torch.int32, device="cuda"),
                                torch.zeros(n, dtype=torch.int32, device="cuda"), d_way)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "lscqp_grid_fields_missions_device" in str(e.value)
    with pytest.raises(api.LscqpError):
        grid.mission_status(2)
    # ... and a decision over another partition than the fields were made for: the copies were cleared for other agents
    d_f, d_i = grid.fields_missions([0, 4, 10], d_s, d_g)
    for other in ([0, 5, 10], [0, 10], [0, 4, 7, 10]):
        with pytest.raises(api.LscqpError) as e:
            grid.waypoints_missions(other, 3.0, 10, 2, WD.dev(torch, np.zeros((n, 9))), None, d_s, d_f, d_i, d_way)
        assert e.value.code == api.ERR_INVALID_ARGUMENT and "same partition" in str(e.value), other
    grid.waypoints_missions([0, 4, 10], 3.0, 10, 2, WD.dev(torch, np.zeros((n, 9))), None, d_s, d_f, d_i, d_way)
    torch.cuda.synchronize()
    assert grid.mission_status(2).tolist() == [0, 0]
    grid.close()
    wmap.close()
    sol.close()


def test_closed_loop_tool_flies_missions_in_one_plan():
    """tools/closed_loop.py missions=K: the summary stays JSON, has one record per mission, and mission 0 -- the world's own, whatever
    flies around it -- holds the bars of test_closed_loop.py::test_forest10_closed_loop_is_safe_and_feasible."""
    import json
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import closed_loop

    log = closed_loop.run(os.path.join(ROOT, "tests", "golden", "forest10_world.json"), steps=60, missions=3)
    back = json.loads(json.dumps(log))
    assert back["missions"] == 3 and back["agents"] == 30 and [m["mission"] for m in back["per_mission"]] == [0, 1, 2]
    assert all(m["walk_bound_reached"] == 0 and m["agents"] == 10 for m in log["per_mission"]) and log["graph_nodes"] > 0
    m0 = log["per_mission"][0]
    assert m0["qp_failed"] == 0 and m0["invalid"] == 0 and m0["truncated_agent_steps"] == 0, m0
    assert m0["min_safety_ratio"] >= 1.0 - 5e-6 and m0["max_vel_excess"] <= 1e-5 and m0["max_acc_excess"] <= 1e-5, m0
    assert m0["mean_progress_m"] > 1.5 and m0["waypoints_updated"] > 50, m0
