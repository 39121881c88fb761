"""Plans whose missions fly over their own worlds (lscqp_plan_set_worlds; include/lscqp.h, "each mission over its own world") against plans of
each mission alone over its own map -- the reference's default configuration as tests/test_missions_gpu.py::_plan builds it: CLSC, FROM_HULL,
goal LP, waypoint_mode GRID_PIBT, M = 10, 2-D, closed loop.  Every comparison is the bits of a buffer or of a record."""
import numpy as np
import pytest

from tests import waypoint_device as WD
from tests import world_cases as WLD

pytestmark = pytest.mark.gpu
SIZES = [10, 6, 12]  # three missions of unequal size over the first three fixture worlds
_CACHE = {}


def _plan(api, sol, wmap, W, N, n_obs=9, constraint_mode=None, **kw):
    return api.Plan(sol, wmap, N, n_obs, WD.agents(api, W["radius"], N), constraint_mode=api.GEN_CLSC if constraint_mode is None else constraint_mode,
                    sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True, z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1,
                    waypoint_mode=api.WAYPOINT_GRID_PIBT, **kw)


def _snapshot(api, plan, n):
    out = {}
    for b in range(19):
        a = plan.get(b)
        out[b] = a.copy() if b in (api.PLAN_GROUP, api.PLAN_SAFETY) else np.ascontiguousarray(a).view(np.uint8).reshape(n, -1).copy()
    return out


def _slice_of(api, snap, sl, base):
    """Mission slice of a snapshot, the two buffers that hold agent ids made local to the mission."""
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


def _setup(api):
    """Solver, the three maps, the missions -- made once.  The maps are shared by every plan of the module (plans prepare them, which changes
    no box)."""
    if not _CACHE:
        g = WLD.fixture()
        W = WLD.world(0, g)
        sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
        maps = [api.WorldMap(g["worlds"][k], W["world_min"], W["world_max"], W["resolution"], W["max_dist"]) for k in range(len(SIZES))]
        off, starts, goals = WLD.seeded_missions(SIZES, seed=1, g=g)
        _CACHE.update(g=g, W=W, sol=sol, maps=maps, off=off, starts=starts, goals=goals)
    c = _CACHE
    return c["W"], c["sol"], c["maps"], c["off"], c["starts"], c["goals"]


def _single_traces(api, torch, steps=30):
    """Every mission alone over its own map, `steps` closed-loop replans through the graph: the reference of the module, flown once."""
    W, sol, maps, off, starts, goals = _setup(api)
    if "single" not in _CACHE:
        traces = []
        for k, sl in enumerate(WLD.slices(off)):
            one = _plan(api, sol, maps[k], W, SIZES[k])
            traces.append(_fly(api, torch, one, SIZES[k], steps, True, starts[sl], goals[sl]))
            assert one.mission_status().tolist() == [0]
            _CACHE.setdefault("single_nodes", one.graph_nodes())
            one.close()
        _CACHE["single"] = traces
    return _CACHE["single"]


def _check_against_singles(api, got, singles, off, steps, what):
    for k, sl in enumerate(WLD.slices(off)):
        for t in range(steps):
            diff = _same(_slice_of(api, got[t], sl, int(off[k])), _slice_of(api, singles[k][t], slice(0, sl.stop - sl.start), 0))
            assert not diff, (what, k, t, diff)


def _worlds_plan(api, n_obs=9, constraint_mode=None):
    W, sol, maps, off, _, _ = _setup(api)
    ws = api.Worlds(maps)
    plan = _plan(api, sol, maps[0], W, int(off[-1]), n_obs=n_obs, constraint_mode=constraint_mode, mission_offsets=off)
    plan.set_worlds(ws)
    return plan, ws


def test_missions_over_their_own_worlds_fly_as_their_own_plans_would(api, torch_cuda):
    """Missions of 10, 6 and 12 agents over three fixture worlds, 30 closed-loop replans: eager equals graph, every mission's slice of every
    buffer equals a plan of that mission alone over its own map replan by replan, no walk reaches its bound -- and the worlds matter: mission
    1's corridors after the first replan are not the ones the same mission gets over world 0."""
    torch = torch_cuda
    W, sol, maps, off, starts, goals = _setup(api)
    steps, N = 30, int(off[-1])
    singles = _single_traces(api, torch, steps)
    flights = {}
    for graph in (False, True):
        plan, ws = _worlds_plan(api)
        flights[graph] = _fly(api, torch, plan, N, steps, graph, starts, goals)
        assert not plan.mission_status().any() and (plan.graph_nodes() > 0) == graph
        plan.close()
        ws.close()
    for t in range(steps):
        assert not _same(flights[False][t], flights[True][t]), t
    _check_against_singles(api, flights[True], singles, off, steps, "worlds")
    moved = sum(int(s[api.PLAN_WAYPOINT_UPDATED].view(np.int32).sum()) for s in flights[True])
    assert moved > 50, moved
    sl = WLD.slices(off)[1]
    wrong = _plan(api, sol, maps[0], W, SIZES[1])  # mission 1 over world 0
    other = _fly(api, torch, wrong, SIZES[1], 1, False, starts[sl], goals[sl])
    wrong.close()
    assert not np.array_equal(other[0][api.PLAN_SFC], flights[True][0][api.PLAN_SFC][sl])


def test_another_partition_of_the_same_count_moves_agents_to_the_world_of_their_new_mission(api, torch_cuda):
    """set_missions with the same count and other offsets AFTER set_worlds: [0, 10, 16, 28] becomes [0, 14, 16, 28], so agents 10 .. 13 leave
    mission 1 for mission 0 -- for the grid, the neighbours, the record AND the corridors: every slice equals a plan of the new mission alone
    over its own map.  Those four were drawn for world 1: in world 0 some of them get other corridors or none, which is what a stale index
    would hide."""
    torch = torch_cuda
    W, sol, maps, off, starts, goals = _setup(api)
    off2, steps, N = np.array([0, 14, 16, 28]), 8, int(off[-1])
    for sl in WLD.slices(off2):  # (PIBT's precondition within the new missions: distinct start nodes)
        assert len({tuple(p) for p in starts[sl]}) == sl.stop - sl.start
    singles = []
    for k, sl in enumerate(WLD.slices(off2)):
        one = _plan(api, sol, maps[k], W, sl.stop - sl.start)
        singles.append(_fly(api, torch, one, sl.stop - sl.start, steps, True, starts[sl], goals[sl]))
        one.close()
    plan, ws = _worlds_plan(api)  # (the old partition, flown one replan by a plan of its own: a reset leaves the corridor buffer alone)
    before = _fly(api, torch, plan, N, 1, True, starts, goals)
    plan.close()
    ws.close()
    plan, ws = _worlds_plan(api)
    plan.set_missions(off2)
    with pytest.raises(api.LscqpError):
        plan.step()
    got = _fly(api, torch, plan, N, steps, True, starts, goals)
    assert plan.missions().tolist() == off2.tolist() and not plan.mission_status().any()
    _check_against_singles(api, got, singles, off2, steps, "new partition")
    moved = slice(10, 14)  # the agents that changed world: their first corridors are not the ones world 1 gave them
    assert not np.array_equal(before[0][api.PLAN_SFC][moved], got[0][api.PLAN_SFC][moved])
    plan.close()
    ws.close()


def _record_bytes(rec, base):
    r = rec.copy()
    for f in ("safety_agent", "safety_other"):
        r[f] = np.where(r[f] >= 0, r[f] - base, r[f])
    return r.tobytes()


def test_records_of_missions_over_their_own_worlds(api, torch_cuda):
    """lscqp_plan_run to at most 60 replans: the three records equal those of the three single plans (agent ids relative to the mission)."""
    W, sol, maps, off, starts, goals = _setup(api)
    plan, ws = _worlds_plan(api)
    plan.set_record(0.1)
    plan.reset(starts, goals)
    flown = plan.run(60, check_every=1, graph=True)
    rec, dist = plan.record().download()
    plan.close()
    ws.close()
    assert 1 <= flown <= 60
    for k, sl in enumerate(WLD.slices(off)):
        one = _plan(api, sol, maps[k], W, SIZES[k])
        one.set_record(0.1)
        one.reset(starts[sl], goals[sl])
        one.run(60, check_every=1, graph=True)
        r1, d1 = one.record().download()
        one.close()
        assert _record_bytes(rec[k:k + 1], int(off[k])) == _record_bytes(r1, 0), (k, rec[k], r1)
        assert np.array_equal(dist[sl], d1), k
    assert (rec["distance"] > 1.0).all()


def test_a_shared_obstacle_over_the_worlds(api, torch_cuda):
    """One straight obstacle shared by all missions, constraint_mode LSC, 10 replans: every slice equals the single plan with that obstacle."""
    torch = torch_cuda
    W, sol, maps, off, starts, goals = _setup(api)
    models = api.obstacle_models([dict(type="straight", start=[-4.0, 3.0, W["z_2d"]], goal=[4.0, -3.0, W["z_2d"]], size=0.2, speed=0.6, max_acc=1.0)])
    plan, ws = _worlds_plan(api, constraint_mode=api.GEN_LSC)
    plan.set_obstacles(models)
    got = _fly(api, torch, plan, int(off[-1]), 10, True, starts, goals)
    table = plan.get_obstacles()
    plan.close()
    ws.close()
    singles = []
    for k, sl in enumerate(WLD.slices(off)):
        one = _plan(api, sol, maps[k], W, SIZES[k], constraint_mode=api.GEN_LSC)
        one.set_obstacles(models)
        singles.append(_fly(api, torch, one, SIZES[k], 10, True, starts[sl], goals[sl]))
        assert one.get_obstacles().tobytes() == table.tobytes()
        one.close()
    _check_against_singles(api, got, singles, off, 10, "obstacle")
    assert np.abs(table["position"][0][:2] - np.array([-4.0, 3.0])).max() > 0.5  # (it moved)


def test_plan_refusals(api, torch_cuda):
    W, sol, maps, off, starts, goals = _setup(api)
    ws3, ws2 = api.Worlds(maps), api.Worlds(maps[:2])
    N = int(off[-1])

    def refused(call, text, code=api.ERR_INVALID_ARGUMENT):
        with pytest.raises(api.LscqpError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)

    plan = _plan(api, sol, maps[0], W, N)
    refused(lambda: plan.set_worlds(ws3), "no mission partition")
    plan.set_missions(off)
    refused(lambda: plan.set_worlds(ws2), "2 worlds for 3 missions")
    # the shape: a world box one metre higher, and a coarser map
    for kw, field in ((dict(world_max=[5.0, 5.0, 3.5]), "world_max"), (dict(resolution=0.2), "resolution")):
        args = dict(world_min=W["world_min"], world_max=W["world_max"], resolution=W["resolution"], max_dist=W["max_dist"])
        args.update(kw)
        odd = [api.WorldMap(W["boxes"], **args) for _ in range(3)]
        wso = api.Worlds(odd)
        refused(lambda: plan.set_worlds(wso), "differ from the map the plan was created with in " + field)
        wso.close()
        for m in odd:
            m.close()
    assert plan.missions().tolist() == off.tolist()
    plan.reset(starts, goals)
    plan.step()  # (every refusal left the plan as it was: one map, steppable)
    plan.set_worlds(ws3)
    for graph in (False, True):
        refused(lambda: plan.step(graph=graph), "lscqp_plan_set_worlds: lscqp_plan_reset must come")
    refused(lambda: plan.set_missions([0, 14, N]), "3 worlds")
    refused(lambda: plan.set_missions(None), "3 worlds")
    plan.set_missions(off)  # (the same count passes)
    plan.reset(starts, goals)
    plan.step(graph=True)
    plan.close()
    # a class without corridors
    sol0 = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, use_sfc=False, world_min=W["world_min"], world_max=W["world_max"]))
    bare = api.Plan(sol0, None, N, 9, WD.agents(api, W["radius"], N), constraint_mode=api.GEN_CLSC, z_2d=W["z_2d"], mission_offsets=off)
    refused(lambda: bare.set_worlds(ws3), "no corridors")
    bare.close()
    sol0.close()
    ws3.close()
    ws2.close()


def test_back_to_one_map_and_compositions(api, torch_cuda):
    """set_worlds(None) + reset: the buffers and the graph of a partition plan that never saw the call.  set_grid after set_worlds keeps the
    worlds.  A member map prepared again after the capture: the flight goes on as the single plans'.  The missions of this test start on
    nodes that are free in EVERY world: lscqp_plan_reset leaves the corridor buffer alone and a refused initializeSFC keeps what it finds
    there, so only agents that every map admits make a plan's history invisible after a reset."""
    torch = torch_cuda
    W, sol, maps, off, _, _ = _setup(api)
    _, starts, goals = WLD.seeded_missions(SIZES, seed=2, g=_CACHE["g"], free_everywhere=True)
    N, steps, more_steps = int(off[-1]), 8, 4
    singles = []
    for k, sl in enumerate(WLD.slices(off)):
        one = _plan(api, sol, maps[k], W, SIZES[k])
        singles.append(_fly(api, torch, one, SIZES[k], steps + more_steps, True, starts[sl], goals[sl]))
        one.close()
    never = _plan(api, sol, maps[0], W, N, mission_offsets=off)
    ref = _fly(api, torch, never, N, steps, True, starts, goals)
    nodes = never.graph_nodes()
    never.close()
    assert all((s[api.PLAN_SFC_STATUS].view(np.int32) == 1).all() for s in ref[:1])  # (every initializeSFC over world 0 succeeds)
    plan, ws = _worlds_plan(api)
    got = _fly(api, torch, plan, N, steps, True, starts, goals)
    assert plan.graph_nodes() == nodes  # (the worlds launch takes the place of the corridor node: the chain is as long)
    _check_against_singles(api, got, singles, off, steps, "before")
    assert any(_same(a, b) for a, b in zip(got, ref))
    plan.set_worlds(None)
    with pytest.raises(api.LscqpError):
        plan.step()
    back = _fly(api, torch, plan, N, steps, True, starts, goals)
    for t, (a, b) in enumerate(zip(back, ref)):
        assert not _same(a, b), (t, _same(a, b))
    assert plan.graph_nodes() == nodes
    # set_grid after set_worlds
    plan.set_worlds(ws)
    api._call("lscqp_plan_set_grid", plan._p, 0.5)
    grid = plan.grid()
    alone = api.Grid(maps[2], 0.5, W["radius"], W["z_2d"])
    assert np.array_equal(grid.download_world(2), alone.download())
    alone.close()
    got = _fly(api, torch, plan, N, steps, True, starts, goals)
    _check_against_singles(api, got, singles, off, steps, "set_grid")
    # a member prepared for larger agents after the capture: its generation moves, the plan drops its graph and flies on -- correctly
    assert plan.graph_nodes() > 0
    maps[1].prepare(0.45)
    more = []
    for _ in range(more_steps):
        plan.step(graph=True)
        torch.cuda.synchronize()
        more.append(_snapshot(api, plan, N))
    for k, sl in enumerate(WLD.slices(off)):
        for t in range(more_steps):
            diff = _same(_slice_of(api, more[t], sl, int(off[k])), _slice_of(api, singles[k][steps + t], slice(0, SIZES[k]), 0))
            assert not diff, ("prepared again", k, t, diff)
    plan.close()
    ws.close()


def test_closed_loop_tool_flies_missions_over_their_own_worlds():
    """tools/closed_loop.py missions=3 with worlds= three fixture worlds (as box lists): the summary stays JSON, names the worlds, has one
    record per mission, every mission's seeded agents start on free nodes of ITS world (no QP fails, nothing invalid, safe), and mission 0 --
    the fixture's own agents over the fixture's first world -- makes progress."""
    import json

    closed_loop = WD.closed_loop()
    g = WLD.fixture()
    log = closed_loop.run(WLD.world(0, g), steps=40, missions=3, worlds=[g["worlds"][k] for k in range(3)])
    back = json.loads(json.dumps(log))
    assert back["missions"] == 3 and back["worlds"] == 3 and back["agents"] == 30 and [m["mission"] for m in back["per_mission"]] == [0, 1, 2]
    assert log["graph_nodes"] > 0 and all(m["walk_bound_reached"] == 0 and m["agents"] == 10 for m in log["per_mission"])
    for m in log["per_mission"]:
        assert m["qp_failed"] == 0 and m["invalid"] == 0 and m["truncated_agent_steps"] == 0, m
        assert m["min_safety_ratio"] >= 1.0 - 5e-6 and m["max_vel_excess"] <= 1e-5 and m["max_acc_excess"] <= 1e-5, m
    assert log["per_mission"][0]["mean_progress_m"] > 1.0 and log["per_mission"][0]["waypoints_updated"] > 20, log["per_mission"][0]
