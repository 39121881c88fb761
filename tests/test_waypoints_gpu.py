"""The grid planner / MAPF layer on the device (lscqp_grid, lscqp_waypoints_device, lscqp_plan's waypoint_mode 1) against the plain Python
restatement of the reference (tests/grid_reference.py).  Everything compared is integers or exact grid points: every comparison is exact
equality.  Invariants of a PIBT step are asserted separately from equality."""
import os

import numpy as np
import pytest

from tests import grid_reference as R
from tests import waypoint_cases as WC
from tests import waypoint_device as WD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _check_invariants(G, label, desired, way):
    """No two agents of a group share a taken node, no swaps, every taken node is the present one or a free 4-neighbour of it."""
    n = len(way)
    cur = [G.node(p) for p in way]
    des = [(int(d) % G.W, int(d) // G.W) for d in desired]
    by_group = {}
    for i in range(n):
        assert abs(des[i][0] - cur[i][0]) + abs(des[i][1] - cur[i][1]) <= 1, i
        assert des[i] == cur[i] or G.free[des[i][1], des[i][0]], i
        by_group.setdefault(int(label[i]), []).append(i)
    for members in by_group.values():
        taken = {des[i]: i for i in members}
        assert len(taken) == len(members)
        at = {cur[i]: i for i in members}
        for i in members:
            j = at.get(des[i])
            assert j is None or j == i or des[j] != cur[i], (i, j)


def _same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def _compare_step(api, torch, grid, G, rng, s, F, init_d, d_field, d_init_d):
    label, desired, updated, new = R.waypoint_step(G, rng, s["positions"], None if s["plans"] is None else list(s["plans"]), s["current_goals"],
                                                   s["waypoints"], F, init_d)
    g, d, u, w = WD.decision_step(torch, grid, rng, s, d_field, d_init_d)
    _check_invariants(G, g, d, s["waypoints"])
    assert np.array_equal(d, desired), np.nonzero(d != desired)
    assert _same_partition(g, label) and np.array_equal(g, label)  # (both name a group by its least id)
    assert np.array_equal(u, updated), np.nonzero(u != updated)
    assert np.array_equal(w, new), np.abs(w - new).max()  # (kept waypoints untouched, new ones the float32 grid points)
    return label, updated


def test_grid_occupancy_equals_the_restatement(api, oracle, torch_cuda):
    for w in (WC.forest10(), WD.closed_loop().random_forest_world(64)):
        wmap, grid = WD.device_grid(api, w)
        G = WC.reference_grid(oracle, w)
        assert grid.dims.tolist() == G.dims and grid.grid_min.tolist() == G.gmin
        occ = grid.download()
        assert occ.shape == G.occ.shape and np.array_equal(occ.astype(bool), G.occ), int((occ.astype(bool) != G.occ).sum())
        grid.close()
        wmap.close()
    assert int(WC.reference_grid(oracle, WC.forest10()).occ.sum()) == 96


def test_fields_equal_the_restatement(api, oracle, torch_cuda):
    import torch

    for w in (WC.forest10(), WD.closed_loop().random_forest_world(64)):
        wmap, grid = WD.device_grid(api, w)
        G = WC.reference_grid(oracle, w)
        F, init_d = R.mission_fields(G, w["starts"], w["goals"])
        d_field, d_init_d = WD.device_fields(torch, grid, w["starts"], w["goals"])
        assert np.array_equal(grid.download(mission=True).astype(bool), ~G.free)
        assert np.array_equal(d_field.cpu().numpy(), F)
        assert np.array_equal(d_init_d.cpu().numpy(), init_d)
        grid.close()
        wmap.close()


def test_fields_of_a_grid_too_large_for_lds(api, oracle, torch_cuda):
    """400 x 400 nodes (the LDS form holds 65 000): the same sweeps in HBM.  The occupancy comes from the device here (its rule is tested on
    the smaller worlds; the restatement's node-by-node loop takes minutes at this size), the BFS is the restatement's."""
    import torch

    w = WC.walled_world(400)
    wmap, grid = WD.device_grid(api, w)
    assert grid.dims.tolist() == [400, 400, 1]
    occ = grid.download().astype(bool)
    assert 1000 < occ.sum() < 4000
    G = R.Grid(w["world_min"], w["world_max"], w["z_2d"], 0.5, w["radius"], occ=occ)
    F, init_d = R.mission_fields(G, w["starts"], w["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, w["starts"], w["goals"])
    got = d_field.cpu().numpy()
    assert np.array_equal(got, F)
    assert np.array_equal(d_init_d.cpu().numpy(), init_d)
    # the closed pocket: its nodes hold the sentinel in the fields of the goals outside, and agent 2 (goal inside) cannot be reached from outside
    pi, pj = G.node(w["pocket"])
    assert got[0, pj, pi] == api.GRID_UNREACHABLE and got[1, pj, pi] == api.GRID_UNREACHABLE and got[2, pj, pi] == 0
    assert init_d[2] == api.GRID_UNREACHABLE and 0 < init_d[0] < 2000
    grid.close()
    wmap.close()


def test_waypoints_on_forest10_along_a_rollout(api, oracle, torch_cuda):
    import torch

    w = WC.forest10()
    wmap, grid = WD.device_grid(api, w)
    G = WC.reference_grid(oracle, w)
    F, init_d = R.mission_fields(G, w["starts"], w["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, w["starts"], w["goals"])
    n_updated, n_groups = 0, set()
    for s in WC.seeded_states(G, w, F, init_d, 30, 3.0, seed=3):
        label, updated = _compare_step(api, torch, grid, G, 3.0, s, F, init_d, d_field, d_init_d)
        n_updated += int(updated.sum())
        n_groups.add(len(set(label.tolist())))
    assert n_updated > 30 and len(n_groups) > 1  # the filter both passes and refuses, and the swarm splits and joins along the way
    grid.close()
    wmap.close()


@pytest.mark.parametrize("n_agents", [64, 512])
def test_waypoints_on_random_forests(api, oracle, torch_cuda, n_agents):
    """One group (range -1, and 3 m), a few (2 m, the 512 agents: ~30) and many (1 m: mostly agents alone) on 64 agents swapping sides of a
    circle and on 512 agents between random nodes of a denser forest."""
    import torch

    w = WD.closed_loop().random_forest_world(64) if n_agents == 64 else WC.random_mission(512)
    wmap, grid = WD.device_grid(api, w)
    G = WC.reference_grid(oracle, w)
    F, init_d = R.mission_fields(G, w["starts"], w["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, w["starts"], w["goals"])
    assert np.array_equal(d_init_d.cpu().numpy(), init_d)
    seen = {}
    for rng in (-1, 3.0, 2.0, 1.0):
        for s in WC.seeded_states(G, w, F, init_d, 4 if n_agents == 64 else 2, rng, seed=11):
            label, _ = _compare_step(api, torch, grid, G, rng, s, F, init_d, d_field, d_init_d)
            seen[rng] = len(set(label.tolist()))
    assert seen[-1] == 1 and seen[1.0] > seen[3.0] >= 1 and seen[1.0] > n_agents // 8, seen
    assert n_agents == 64 or 1 < seen[2.0] < seen[1.0], seen
    grid.close()
    wmap.close()


@pytest.mark.parametrize("name", sorted(WC.TOYS))
def test_waypoints_on_toy_cases(api, oracle, torch_cuda, name):
    import torch

    c = WC.toy_case(name)
    wmap, grid = WD.device_grid(api, c["world"])
    assert np.array_equal(grid.download().astype(bool), c["world"]["occ"])
    G = WC.reference_grid(oracle, c["world"])
    F, init_d = R.mission_fields(G, c["starts"], c["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, c["starts"], c["goals"])
    assert np.array_equal(d_field.cpu().numpy(), F) and np.array_equal(d_init_d.cpu().numpy(), init_d)
    if c["init_d"] is not None:
        init_d = np.array(c["init_d"])
        d_init_d = WD.dev(torch, init_d, np.int32)
    s = dict(positions=c["positions"], plans=None, current_goals=c["current_goals"], waypoints=c["waypoints"])
    _compare_step(api, torch, grid, G, c["range"], s, F, init_d, d_field, d_init_d)
    _, d, _, _ = WD.decision_step(torch, grid, c["range"], s, d_field, d_init_d)
    assert d.tolist() == c["expect"]
    grid.close()
    wmap.close()


def _plan_points(x, N, M, z):
    X = x.reshape(N, 2, M, 6)
    pts = np.zeros((N, M + 1, 3))
    pts[:, :M, :2] = X[:, :, :, 0].transpose(0, 2, 1)
    pts[:, M, :2] = X[:, :, M - 1, 5]
    pts[..., 2] = np.float32(z)
    return pts


def test_forest10_flies_from_starts_and_goals_alone(api, oracle, torch_cuda):
    """forest10 through Plan(waypoint_mode=1, closed_loop=True): 79 replans with no host work between them, eagerly and as one captured graph
    per replan, bit-identical in every buffer.  After every replan the waypoint buffer equals the restatement fed with the state, plans and
    goal points the replan before left.  Held to the bars of test_closed_loop.py::test_forest10_closed_loop_is_safe_and_feasible."""
    import torch

    W = WC.forest10()
    N, M, K = 10, 10, 79
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    G = WC.reference_grid(oracle, W)
    F, init_d = R.mission_fields(G, W["starts"], W["goals"])
    BUFS = [b for b in range(19) if b not in (api.PLAN_HEADER, api.PLAN_ROWS, api.PLAN_SFC, api.PLAN_INFO, api.PLAN_SAFETY)]
    RAW = (api.PLAN_HEADER, api.PLAN_ROWS, api.PLAN_SFC, api.PLAN_INFO, api.PLAN_SAFETY)
    flights = {}
    for graph in (False, True):
        sol, wmap, plan = WD.forest10_plan(api, W, api.WAYPOINT_GRID_PIBT)
        plan.reset(starts, goals)
        assert np.array_equal(plan.get(api.PLAN_WAYPOINT).reshape(N, 3), np.float32(starts).astype(float))
        assert np.array_equal(plan.get(api.PLAN_DESIRED_GOAL).reshape(N, 3), np.float32(goals).astype(float))
        pg = plan.grid()
        assert np.array_equal(pg.download().astype(bool), G.occ) and pg.dims.tolist() == G.dims
        log = dict(failed=0, invalid=0, min_ratio=np.inf, vel=0.0, acc=0.0, updated=0)
        trace = []
        for k in range(K):
            state, x, cg, way = (plan.get(b) for b in (api.PLAN_STATE, api.PLAN_PLAN, api.PLAN_GOAL, api.PLAN_WAYPOINT))
            state, cg, way = state.reshape(N, 9), cg.reshape(N, 3), way.reshape(N, 3)
            label, desired, updated, new = R.waypoint_step(G, 3.0, state[:, :3], list(_plan_points(x, N, M, W["z_2d"])), cg, way, F, init_d)
            plan.step(graph=graph)
            torch.cuda.synchronize()
            assert pg.status() == 0
            assert np.array_equal(plan.get(api.PLAN_WAYPOINT).reshape(N, 3), new), k
            assert np.array_equal(plan.get(api.PLAN_WAYPOINT_UPDATED), updated) and np.array_equal(plan.get(api.PLAN_GROUP), label), k
            hdr = plan.get(api.PLAN_HEADER)
            assert np.array_equal(hdr["next_waypoint"], new)  # the QP of this replan flew towards it
            st, valid, saf = plan.get(api.PLAN_STATUS), plan.get(api.PLAN_VALID), plan.get(api.PLAN_SAFETY)
            log["failed"] += int((st != 0).sum())
            log["invalid"] += int(((st == 0) & (valid != 1)).sum())
            log["min_ratio"] = min(log["min_ratio"], float(saf["safety_ratio"].min()))
            log["vel"], log["acc"] = max(log["vel"], float(saf["vel_excess_ratio"].max())), max(log["acc"], float(saf["acc_excess_ratio"].max()))
            log["updated"] += int(updated.sum())
            trace.append([plan.get(b).copy() for b in BUFS] + [plan.get(b).view(np.uint8).copy() for b in RAW])
        state = plan.get(api.PLAN_STATE).reshape(N, 9)
        log["mean_progress_m"] = float((np.linalg.norm(goals[:, :2] - starts[:, :2], axis=1) - np.linalg.norm(goals[:, :2] - state[:, :2], axis=1)).mean())
        log["graph_nodes"] = plan.graph_nodes()
        print("waypoint_mode 1, %s: %s" % ("graph" if graph else "eager", log))
        flights[graph] = (trace, log)
        plan.close()
        wmap.close()
    for k in range(K):
        for a, b in zip(flights[False][0][k], flights[True][0][k]):
            assert np.array_equal(a, b), k
    assert flights[False][1]["graph_nodes"] == 0 and flights[True][1]["graph_nodes"] > 0
    for graph in (False, True):
        log = flights[graph][1]
        assert log["failed"] == 0 and log["invalid"] == 0, log
        assert log["min_ratio"] >= 1.0 - 5e-6, log
        assert log["vel"] <= 1e-5 and log["acc"] <= 1e-5, log
        assert log["mean_progress_m"] > 1.5, log
        assert log["updated"] > 100, log


@pytest.mark.parametrize("nodes", [200, 252, 253])
def test_fields_either_side_of_the_lds_limit(api, oracle, torch_cuda, nodes):
    """The field kernel's LDS form beyond the 64 KB a kernel gets by default (200 x 200 nodes: 82 KB; 252 x 252: 129 KB, the largest grid it
    takes, 64 516 padded nodes) and the first grid that goes to the HBM form (253 x 253: 65 025).  Occupancy from the device, as above."""
    import torch

    w = WC.walled_world(nodes)
    wmap, grid = WD.device_grid(api, w)
    assert grid.dims.tolist() == [nodes, nodes, 1]
    G = R.Grid(w["world_min"], w["world_max"], w["z_2d"], 0.5, w["radius"], occ=grid.download().astype(bool))
    F, init_d = R.mission_fields(G, w["starts"], w["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, w["starts"], w["goals"])
    assert np.array_equal(d_field.cpu().numpy(), F)
    assert np.array_equal(d_init_d.cpu().numpy(), init_d)
    assert init_d[2] == api.GRID_UNREACHABLE and 0 < init_d[0] < 2000
    grid.close()
    wmap.close()


@pytest.mark.parametrize("router", ["host", "device"])
def test_closed_loop_tool_with_either_router(router):
    """tools/closed_loop.py: its summary is JSON with either router, names the router it used, and the mission flown with
    lscqp_waypoints_device in place of the host stand-in holds the bars of test_closed_loop.py."""
    import json

    log = WD.closed_loop().run(os.path.join(ROOT, "tests", "golden", "forest10_world.json"), steps=60, router=router)
    back = json.loads(json.dumps(log))
    assert back["router"] == router == log["router"]
    assert log["qp_failed"] == 0 and log["invalid"] == 0 and log["sfc_kept"] == 0, log
    assert log["min_safety_ratio"] >= 1.0 - 5e-6, log
    assert log["max_vel_excess"] <= 1e-5 and log["max_acc_excess"] <= 1e-5, log
    assert log["mean_progress_m"] > 1.5, log
    if router == "device":
        assert log["waypoints_updated"] > 50, log
    with pytest.raises(ValueError):
        WD.closed_loop().run(os.path.join(ROOT, "tests", "golden", "forest10_world.json"), steps=1, router="elsewhere")


def test_range_zero_leaves_every_agent_alone(api, torch_cuda):
    """A class with communication_range 0 (nobody is within it): the plan is created, reset and steps; every agent is its own group."""
    import torch

    W = WC.forest10()
    N = 10
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, comm_range=0.0, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    plan = api.Plan(sol, wmap, N, N - 1, WD.agents(api, W["radius"], N), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, closed_loop=True, z_2d=W["z_2d"],
                    waypoint_mode=api.WAYPOINT_GRID_PIBT)
    plan.reset(np.array(W["starts"], float), np.array(W["goals"], float))
    for _ in range(3):
        plan.step()
    torch.cuda.synchronize()
    assert plan.get(api.PLAN_GROUP).tolist() == list(range(N)) and plan.grid().status() == 0
    assert plan.get(api.PLAN_WAYPOINT_UPDATED).sum() > 0
    plan.close()
    wmap.close()


def test_waypoint_mode_0_is_unchanged(api, torch_cuda):
    """A plan created with waypoint_mode = 0 has the chain it had: the new buffers do not exist, the captured graph has the node count of the
    chain before (10, the number the parent commit's library reports for this plan), and mode 1 adds exactly the two launches of the decision
    in front."""
    import torch

    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    nodes = {}
    for mode in (api.WAYPOINT_FROM_CALLER, api.WAYPOINT_GRID_PIBT):
        sol, wmap, plan = WD.forest10_plan(api, W, mode)
        if mode == api.WAYPOINT_FROM_CALLER:
            for b in (api.PLAN_DESIRED_GOAL, api.PLAN_WAYPOINT_UPDATED, api.PLAN_GROUP):
                assert plan.pointer(b) == (None, 0)
            assert plan.grid() is None
            plan.reset(starts)
            plan.put(api.PLAN_WAYPOINT, starts)
        else:
            plan.reset(starts, goals)
        for _ in range(3):
            plan.step(graph=True)
        torch.cuda.synchronize()
        assert (plan.get(api.PLAN_STATUS) == 0).all()
        nodes[mode] = plan.graph_nodes()
        plan.close()
        wmap.close()
    print("graph nodes: waypoint_mode 0: %d, waypoint_mode 1: %d" % (nodes[0], nodes[1]))
    assert nodes[0] == PARENT_GRAPH_NODES and nodes[1] == nodes[0] + 2


PARENT_GRAPH_NODES = 10  # (what the parent commit's library reports for this plan)


def test_argument_errors(api, torch_cuda):
    W = WC.forest10()
    N = 10
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    with pytest.raises(api.LscqpError) as e:
        api.Grid(wmap, 0.5, 0.15, 0.6, world_dimension=3)
    assert e.value.code == api.ERR_UNSUPPORTED and "2-D" in str(e.value)
    kw = dict(constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, z_2d=W["z_2d"], waypoint_mode=api.WAYPOINT_GRID_PIBT)
    sol2 = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    with pytest.raises(api.LscqpError) as e:  # a shard: not every agent's waypoint and plan is here
        api.Plan(sol2, wmap, 5, 9, WD.agents(api, W["radius"], N), n_total=N, first_agent=0, **kw)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "n_agents == n_total" in str(e.value)
    sol3 = api.Solver(api.make_desc(M=5, dim=3, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    with pytest.raises(api.LscqpError) as e:  # a 3-D class
        api.Plan(sol3, wmap, N, 9, WD.agents(api, W["radius"], N), **kw)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "2-D" in str(e.value)
    nosfc = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, use_sfc=False, world_min=W["world_min"], world_max=W["world_max"]))
    with pytest.raises(api.LscqpError) as e:  # no map
        api.Plan(nosfc, None, N, 9, WD.agents(api, W["radius"], N), **kw)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "needs a map" in str(e.value)
    sol, wmap2, plan = WD.forest10_plan(api, W, api.WAYPOINT_GRID_PIBT)
    with pytest.raises(api.LscqpError) as e:  # the mission's goal points are what the fields are made from
        plan.reset(np.array(W["starts"], float))
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    with pytest.raises(api.LscqpError) as e:  # ... and no step before them
        plan.step()
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "lscqp_plan_reset" in str(e.value)
    plan.close()
    wmap2.close()
    wmap.close()
