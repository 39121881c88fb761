"""Patrol missions inside the replan chain (include/lscqp.h, "patrol missions"; csrc/lscplan.hip, lscpatrol.hip): lscqp_plan_set_patrol on the
smallest missions that turn, against the numpy restatement of the transition (tests/patrol_reference.py), the restatement of the grid
planner fed with each agent's field of the leg it was on (tests/grid_reference.py), twins without a patrol, partitions, the record, and the
life of the option.  Every flight prints the legs its agents completed and requires two of every agent where the exchange-back matters."""
import numpy as np
import pytest

from tests import grid_reference as R
from tests import patrol_reference as PR
from tests import waypoint_cases as WC
from tests import waypoint_device as WD

pytestmark = pytest.mark.gpu
ALL = range(19)
THR = 0.25


def _bufs(plan):
    return [np.ascontiguousarray(plan.get(b)).tobytes() if plan.pointer(b)[1] else b"" for b in ALL]


def _differ(a, b):
    return [k for k, (x, y) in enumerate(zip(a, b)) if x != y]


def _f32(a):
    return np.float32(np.array(a, float)).astype(np.float64)


# ---- (a) static goals, no map, 3-D -------------------------------------------------------------------------------------------------------

def _static_plans(api):
    wmin, wmax = [-4.0, -4.0, 0.0], [4.0, 4.0, 3.0]
    # (communication range 6 m: its rows keep every plan within 3 m of the waypoint, which is the far end of a 2 m leg here)
    sol = api.Solver(api.make_desc(M=5, dim=3, dt=0.2, comm_range=6.0, use_sfc=False, world_min=wmin, world_max=wmax))
    ag = np.zeros(2, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = 0.15, 2.0, 1.0, 2.0, 1.0
    kw = dict(constraint_mode=api.GEN_LSC, optimize_goal=False, closed_loop=True)
    return sol, api.Plan(sol, None, 2, 1, ag, **kw), api.Plan(sol, None, 2, 1, ag, **kw)


def _static_flight(api, torch, graph, replans=70):
    """The patrol plan and its twin, whose goal buffer the test rewrites from the restatement between replans; both get the desired goal as
    their waypoint.  -> (trace of the patrol plan's buffers, legs, graph nodes of both)"""
    starts = np.array([[-1.0, 0.0, 1.0], [0.1, -1.0, 1.3]])
    goals = np.array([[1.0, 0.0, 1.0], [0.1, 1.0, 1.3]])
    sol, pat, twin = _static_plans(api)
    pat.set_patrol(THR)
    with pytest.raises(api.LscqpError, match="goal points"):
        pat.reset(starts)
    for p in (pat, twin):
        p.reset(starts, goals)
    assert pat.patrol(api.PATROL_FIELD).size == 0 and pat.patrol_pointer(api.PATROL_INIT_D_OTHER) == (None, 0)
    assert twin.patrol(api.PATROL_LEGS).size == 0  # (no patrol: no buffers)
    desired, start = _f32(goals), _f32(starts)
    legs, sw = np.zeros(2, np.int32), np.zeros(2, np.int32)
    assert np.array_equal(pat.patrol(api.PATROL_DESIRED), desired) and np.array_equal(pat.patrol(api.PATROL_START), start)
    trace = []
    for r in range(replans):
        state = pat.get(api.PLAN_STATE).reshape(2, 9)
        PR.transition(state, desired, start, THR, 3, 1.0, legs, sw)
        twin.put(api.PLAN_GOAL, desired)
        for p in (pat, twin):
            p.put(api.PLAN_WAYPOINT, desired)
            p.step(graph=graph)
        torch.cuda.synchronize()
        a, b = _bufs(pat), _bufs(twin)
        assert not _differ(a, b), (r, _differ(a, b))
        assert np.array_equal(pat.patrol(api.PATROL_DESIRED), desired) and np.array_equal(pat.patrol(api.PATROL_START), start), r
        assert np.array_equal(pat.patrol(api.PATROL_LEGS), legs) and np.array_equal(pat.patrol(api.PATROL_SWAPPED), sw), r
        assert (pat.get(api.PLAN_STATUS) == 0).all(), r
        trace.append(a)
    nodes = (pat.graph_nodes(), twin.graph_nodes())
    for p in (pat, twin):
        p.close()
    sol.close()
    return trace, legs, nodes


def test_static_goals_equal_a_twin_whose_goals_the_host_rewrites(api, torch_cuda):
    eager, legs_e, nodes_e = _static_flight(api, torch_cuda, False)
    graph, legs_g, nodes_g = _static_flight(api, torch_cuda, True)
    print("(a) legs per agent:", legs_e.tolist(), "graph nodes (patrol, twin):", nodes_g)
    assert (legs_e >= 2).all() and np.array_equal(legs_e, legs_g)
    for r, (a, b) in enumerate(zip(eager, graph)):
        assert not _differ(a, b), (r, _differ(a, b))
    assert nodes_e == (0, 0) and nodes_g[1] > 0 and nodes_g[0] == nodes_g[1] + 1


# ---- the grid missions -------------------------------------------------------------------------------------------------------------------

def _toy():
    """Three agents in forest10's world: agent 0 with the pillar at (1.0, -2.5) between its start and its goal 1.5 m away (it detours through
    the lane y = -3: five nodes), agent 1 down that lane the other way (2 m), agent 2 towards agent 0's goal region (2 m)."""
    W = dict(WC.forest10())
    z = W["z_2d"]
    W["starts"] = [[0.5, -2.5, z], [2.0, -3.0, z], [3.0, -1.0, z]]
    W["goals"] = [[2.0, -2.5, z], [0.0, -3.0, z], [3.0, -3.0, z]]
    return W


def _grid_plan(api, W, copies=1):
    """(two row slots whatever the number of missions: a mission has three agents, and the same kernel instance solves every plan)"""
    N = len(W["starts"]) * copies
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    plan = api.Plan(sol, wmap, N, 2, WD.agents(api, W["radius"], N), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True,
                    closed_loop=True, z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT)
    return sol, wmap, plan


def _plan_points(x, N, M, z):
    X = x.reshape(N, 2, M, 6)
    pts = np.zeros((N, M + 1, 3))
    pts[:, :M, :2] = X[:, :, :, 0].transpose(0, 2, 1)
    pts[:, M, :2] = X[:, :, M - 1, 5]
    pts[..., 2] = np.float32(z)
    return pts


def _grid_flight(api, torch, graph, replans=80):
    W = _toy()
    N, M, z = 3, 10, W["z_2d"]
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    sol, wmap, plan = _grid_plan(api, W)
    plan.set_patrol(THR)
    plan.reset(starts, goals)
    pg = plan.grid()
    G = R.Grid(W["world_min"], W["world_max"], z, 0.5, W["radius"], occ=pg.download().astype(bool))
    node = G.node([1.0, -2.5, z])
    assert G.occ[node[1], node[0]]  # the pillar between agent 0's start and goal
    F0, d0 = R.mission_fields(G, list(starts), list(goals))
    F1, d1 = R.mission_fields(G, list(goals), list(starts))
    F, D = np.stack([F0, F1]).reshape(2, N, -1), np.stack([d0, d1])
    assert (D < R.UNREACHABLE).all() and D[0, 0] > 3  # (agent 0's way round is longer than its 3 nodes as the crow flies)
    desired, start = _f32(goals), _f32(starts)
    legs, sw = np.zeros(N, np.int32), np.zeros(N, np.int32)
    ids = np.arange(N)
    trace = []
    for r in range(replans):
        state, x, cg, way = (plan.get(b) for b in (api.PLAN_STATE, api.PLAN_PLAN, api.PLAN_GOAL, api.PLAN_WAYPOINT))
        state, cg, way = state.reshape(N, 9), cg.reshape(N, 3), way.reshape(N, 3)
        leg = legs % 2  # the leg every agent is on when the decision runs: the transition comes behind it
        label, _, updated, new = R.waypoint_step(G, 3.0, state[:, :3], list(_plan_points(x, N, M, z)), cg, way,
                                                 F[leg, ids].reshape(N, G.H, G.W), D[leg, ids])
        PR.transition(state, desired, start, THR, 2, z, legs, sw)
        plan.step(graph=graph)
        torch.cuda.synchronize()
        assert pg.status() == 0
        assert np.array_equal(plan.get(api.PLAN_WAYPOINT).reshape(N, 3), new), r
        assert np.array_equal(plan.get(api.PLAN_WAYPOINT_UPDATED), updated) and np.array_equal(plan.get(api.PLAN_GROUP), label), r
        assert np.array_equal(plan.patrol(api.PATROL_DESIRED), desired) and np.array_equal(plan.patrol(api.PATROL_START), start), r
        assert np.array_equal(plan.get(api.PLAN_DESIRED_GOAL).reshape(N, 3), desired), r  # (the public buffer reads right)
        assert np.array_equal(plan.patrol(api.PATROL_LEGS), legs) and np.array_equal(plan.patrol(api.PATROL_SWAPPED), sw), r
        now = legs % 2
        assert np.array_equal(plan.patrol(api.PATROL_FIELD), F[now, ids]) and np.array_equal(plan.patrol(api.PATROL_FIELD_OTHER), F[1 - now, ids]), r
        assert np.array_equal(plan.patrol(api.PATROL_INIT_D), D[now, ids]) and np.array_equal(plan.patrol(api.PATROL_INIT_D_OTHER), D[1 - now, ids]), r
        assert (plan.get(api.PLAN_STATUS) == 0).all(), r
        trace.append(_bufs(plan))
    nodes = plan.graph_nodes()
    plan.close()
    wmap.close()
    sol.close()
    return trace, legs, nodes


def _plain_flight(api, torch, W, replans, patrol=None, graph=True, copies=1, offsets=None, disturb=None, churn=False):
    """A grid plan over `copies` of W's mission flown for `replans`; patrol: a threshold or None.  -> (trace, legs or None, graph nodes, SWAPPED per replan)"""
    starts, goals = np.array(W["starts"] * copies, float), np.array(W["goals"] * copies, float)
    sol, wmap, plan = _grid_plan(api, W, copies)
    if offsets is not None:
        plan.set_missions(offsets)
    if churn:  # set, replaced, taken away: a plan that never saw the calls flies the same bytes
        plan.set_patrol(0.5)
        plan.set_patrol(THR)
        plan.set_patrol(None)
    if patrol is not None:
        plan.set_patrol(patrol)
    plan.reset(starts, goals)
    trace, turned = [], []
    for r in range(replans):
        if disturb is not None and r == disturb[0]:
            disturb[1](plan, wmap)
        plan.step(graph=graph)
        torch.cuda.synchronize()
        trace.append(_bufs(plan))
        if patrol is not None:
            turned.append(plan.patrol(api.PATROL_SWAPPED).copy())
    assert not plan.mission_status().any()
    legs = plan.patrol(api.PATROL_LEGS).copy() if patrol is not None else None
    extra = {w: plan.patrol(w).copy() for w in range(api.PATROL_COUNT)} if patrol is not None else None
    nodes = plan.graph_nodes()
    plan.close()
    wmap.close()
    sol.close()
    return trace, legs, nodes, turned, extra


def test_grid_mode_routes_every_agent_by_the_field_of_its_leg(api, torch_cuda):
    eager, legs_e, nodes_e = _grid_flight(api, torch_cuda, False)
    graph, legs_g, nodes_g = _grid_flight(api, torch_cuda, True)
    _, _, nodes_plain, _, _ = _plain_flight(api, torch_cuda, _toy(), 3)
    print("(b) legs per agent:", legs_e.tolist(), "graph nodes (patrol, plain):", (nodes_g, nodes_plain))
    assert (legs_e >= 2).all() and np.array_equal(legs_e, legs_g)
    for r, (a, b) in enumerate(zip(eager, graph)):
        assert not _differ(a, b), (r, _differ(a, b))
    assert nodes_e == 0 and nodes_plain > 0 and nodes_g == nodes_plain + 2


def test_no_effect_while_nobody_turns(api, torch_cuda):
    W = _toy()
    plain, _, _, _, _ = _plain_flight(api, torch_cuda, W, 30)
    zero, legs, _, turned, _ = _plain_flight(api, torch_cuda, W, 30, patrol=0.0)
    assert not legs.any() and not np.array(turned).any()
    for r, (a, b) in enumerate(zip(plain, zero)):
        assert not _differ(a, b), (r, _differ(a, b))
    launch, legs, _, turned, _ = _plain_flight(api, torch_cuda, W, 30, patrol=0.1)  # the launch files' threshold
    first = next((r for r, t in enumerate(turned) if t.any()), len(turned))
    print("(c) threshold 0.1: first turn at replan", first, "legs", legs.tolist())
    for r in range(first):
        assert not _differ(plain[r], launch[r]), (r, _differ(plain[r], launch[r]))


def test_two_missions_equal_two_single_patrol_plans(api, torch_cuda):
    W = _toy()
    n, R_ = 3, 80
    one, legs1, _, _, ex1 = _plain_flight(api, torch_cuda, W, R_, patrol=THR)
    two, legs2, _, _, ex2 = _plain_flight(api, torch_cuda, W, R_, patrol=THR, copies=2, offsets=[0, n, 2 * n])
    print("(d) legs per agent:", legs2.tolist())
    assert (legs2 >= 2).all() and np.array_equal(legs2, np.tile(legs1, 2))
    free = [b for b in ALL if b not in (api.PLAN_GROUP, api.PLAN_SAFETY)]  # (the buffers that hold no agent ids)
    for r in range(R_):
        for b in free:
            assert two[r][b] == one[r][b] * 2, (r, b)
        g1, g2 = np.frombuffer(one[r][api.PLAN_GROUP], np.int32), np.frombuffer(two[r][api.PLAN_GROUP], np.int32)
        assert np.array_equal(g2, np.concatenate([g1, g1 + n])), r
        s1, s2 = np.frombuffer(one[r][api.PLAN_SAFETY], api.SAFETY_DTYPE), np.frombuffer(two[r][api.PLAN_SAFETY], api.SAFETY_DTYPE)
        up = s1.copy()
        up["closest_agent"] = np.where(s1["closest_agent"] >= 0, s1["closest_agent"] + n, s1["closest_agent"])
        assert s2.tobytes() == s1.tobytes() + up.tobytes(), r
    for w in range(api.PATROL_COUNT):
        assert np.array_equal(ex2[w], np.concatenate([ex1[w], ex1[w]])), w


def test_a_patrol_never_finishes_and_runs_to_max_replans(api, torch_cuda):
    torch = torch_cuda
    W = _toy()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    out = {}
    for how in ("run", "eager"):
        sol, wmap, plan = _grid_plan(api, W)
        plan.set_record(0.1)
        plan.set_flight_log(64)
        plan.set_patrol(THR)
        plan.reset(starts, goals)
        if how == "run":
            assert plan.run(64, check_every=16) == 64
        else:
            for _ in range(64):
                plan.step()
        torch.cuda.synchronize()
        rec, dist = plan.record().download()
        rows, over = plan.record().log_rows()
        assert (rec["finished"][0], rec["replans"][0], rec["flight_time"][0]) == (0, 64, -1.0) and plan.record().unfinished() == 1
        assert list(rows) == [64] and not any(over) and rec["distance"][0] > 2.0
        assert plan.grid().status() == 0
        out[how] = (_bufs(plan), plan.patrol(api.PATROL_LEGS).copy(), rec.tobytes(), dist.tobytes())
        plan.close()
        wmap.close()
        sol.close()
    print("(e) legs per agent:", out["run"][1].tolist())
    assert (out["run"][1] >= 2).all() and np.array_equal(out["run"][1], out["eager"][1])
    assert not _differ(out["run"][0], out["eager"][0]) and out["run"][2:] == out["eager"][2:]


def test_the_life_of_the_option(api, torch_cuda):
    torch = torch_cuda
    W = _toy()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    sol, wmap, plan = _grid_plan(api, W)
    plan.reset(starts, goals)
    plan.step()
    plan.step(graph=True)
    torch.cuda.synchronize()
    assert plan.graph_nodes() > 0
    for thr in (-0.1, float("nan"), float("inf")):
        with pytest.raises(api.LscqpError, match="goal_threshold"):
            plan.set_patrol(thr)
    plan.step(graph=True)  # (a refused call left the plan as it was, its graph included)
    assert plan.graph_nodes() > 0
    for thr in (THR, 0.5, None):  # set, replace, clear
        plan.set_patrol(thr)
        assert plan.graph_nodes() == 0
        for graph in (False, True):
            with pytest.raises(api.LscqpError, match="lscqp_plan_set_patrol: lscqp_plan_reset must come before the next step") as e:
                plan.step(graph=graph)
            assert e.value.code == api.ERR_INVALID_ARGUMENT and not torch.cuda.is_current_stream_capturing()
        plan.reset(starts, goals)
        plan.step()
        plan.step(graph=True)
        torch.cuda.synchronize()
        assert plan.graph_nodes() > 0
    plan.close()
    wmap.close()
    sol.close()
    sharded = api.Plan(*_sharded_args(api, W), n_total=3, first_agent=0, constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, z_2d=W["z_2d"])
    with pytest.raises(api.LscqpError, match="n_agents == n_total"):
        sharded.set_patrol(0.1)
    sharded.close()
    # a plan from which the patrol was taken away flies the bytes of one that never saw the call
    never, _, nodes_never, _, _ = _plain_flight(api, torch, W, 12)
    taken, _, nodes_taken, _, _ = _plain_flight(api, torch, W, 12, churn=True)
    assert nodes_never == nodes_taken
    for r, (a, b) in enumerate(zip(never, taken)):
        assert not _differ(a, b), (r, _differ(a, b))


def test_closed_loop_tool_flies_a_patrol():
    """tools/closed_loop.py patrol=T: the summary stays JSON and carries the legs per agent, per mission, and their sum; the chain has the two
    nodes more.  (Mission 0 is forest10's own: its 8 m legs do not end within 12 replans.  A seeded mission may hold a short leg.)"""
    import json
    import os

    world = os.path.join(WD.ROOT, "tests", "golden", "forest10_world.json")
    log = WD.closed_loop().run(world, steps=12, missions=2, patrol=0.1)
    back = json.loads(json.dumps(log))
    legs = [m["legs"] for m in back["per_mission"]]
    print("tool: legs per mission", legs)
    assert back["patrol_goal_threshold"] == 0.1 and legs[0] == [0] * 10 and len(legs[1]) == 10 and all(isinstance(v, int) and v >= 0 for v in legs[1])
    assert back["legs"] == sum(legs[1])
    plain = WD.closed_loop().run(world, steps=12, missions=2)
    assert "legs" not in plain and plain["graph_nodes"] + 2 == log["graph_nodes"]
    one = WD.closed_loop().run(world, steps=3, patrol=0.1)  # (without missions: one mission in one plan)
    assert one["missions"] == 1 and one["per_mission"][0]["legs"] == [0] * 10


def _sharded_args(api, W):
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    return sol, wmap, 2, 2, WD.agents(api, W["radius"], 3)


def test_a_map_that_moves_while_agents_are_on_different_legs(api, torch_cuda):
    """The map's generation is bumped (a free-space table for larger agents: the corridors are the same) at the first replan at which the
    agents' leg parities differ: the plan drops its graph, rebuilds its grid and BOTH legs' fields from the buffers as they stand, and flies on
    byte for byte as the undisturbed plan does."""
    W = _toy()
    R_ = 80
    calm, legs, _, turned, ex = _plain_flight(api, torch_cuda, W, R_, patrol=THR)
    par = np.cumsum(np.array(turned), axis=0) % 2
    mixed = [r for r in range(R_ - 10) if 0 < par[r].sum() < 3]
    assert mixed, "no replan with agents on different legs"
    at = mixed[0] + 1
    seen = []

    def bump(plan, wmap):
        seen.append(plan.graph_nodes())
        wmap.prepare(0.45)

    moved, legs_m, nodes, _, ex_m = _plain_flight(api, torch_cuda, W, R_, patrol=THR, disturb=(at, bump))
    print("(f) map moved in front of replan", at, "leg parities", par[at - 1].tolist(), "legs", legs_m.tolist())
    assert seen and seen[0] > 0 and nodes > 0 and np.array_equal(legs, legs_m) and (legs >= 2).all()
    for r, (a, b) in enumerate(zip(calm, moved)):
        assert not _differ(a, b), (r, _differ(a, b))
    for w in range(api.PATROL_COUNT):
        assert np.array_equal(ex[w], ex_m[w]), w
