"""A mission's own obstacles inside the replan chain (include/lscqp.h, "a mission's own obstacles": lscqp_plan_set_mission_obstacles;
csrc/lscplan.hip).  forest10's map and agents cut into two or three missions of at most six agents, the reference's default configuration as
tests/test_record_obstacles_plan_gpu.py builds it (FROM_HULL corridors, goal LP, the device's own waypoints, M = 10, 2-D, closed loop), LSC
and CLSC rows, thirty replans; N_OBS = 7 row slots per agent in every plan, so that a mission alone has the row layout it has in the
partition.  Every comparison is the bytes of a buffer or of a record.  The flights are made once per module and left unchanged."""
import numpy as np
import pytest

from tests import mission_obstacles_cases as MC
from tests import record_obstacles_cases as RC
from tests import record_reference as RR
from tests import waypoint_device as WD
from tests import world_cases as WLD

pytestmark = pytest.mark.gpu

SIZES = (4, 3, 3)
K_REPLANS = MC.N_REPLANS


@pytest.fixture(scope="module")
def env(api, torch_cuda):
    W, off, starts, goals = MC.forest_missions(SIZES)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    yield dict(W=W, sol=sol, wmap=wmap, off=off, starts=starts, goals=goals, n=int(off[-1]), sl=WLD.slices(off))
    wmap.close()
    sol.close()


def make_plan(api, env, mode, n, offsets=None, wmap=None, n_obs=MC.N_OBS):
    W = env["W"]
    return api.Plan(env["sol"], env["wmap"] if wmap is None else wmap, n, n_obs, WD.agents(api, W["radius"], n), constraint_mode=mode, sfc_mode=api.SFC_FROM_HULL,
                    optimize_goal=True, closed_loop=True, z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT,
                    mission_offsets=offsets)


def snapshot(api, plan, n):
    """Every plan buffer per agent ([n][bytes]; the two that hold agent ids as they are) and the three obstacle buffers."""
    out = {}
    for b in range(19):
        a = plan.get(b)
        out[b] = a.copy() if b in (api.PLAN_GROUP, api.PLAN_SAFETY) else np.ascontiguousarray(a).view(np.uint8).reshape(n, -1).copy()
    out["table"], out["obs_safety"], out["clock"] = (plan.get_obstacles(w).copy() for w in (api.PLAN_OBS_TABLE, api.PLAN_OBS_SAFETY, api.PLAN_OBS_CLOCK))
    return out


def mission_slice(api, snap, sl, base, osl=None, k=None):
    """One mission's slice of a snapshot as bytes per buffer, the agent ids made local; osl: its slice of the obstacle table, k: its clock."""
    out = {}
    for b, a in snap.items():
        if b == "table":
            v = a if osl is None else a[osl]
        elif b == "clock":
            v = a if k is None else a[k:k + 1]
        else:
            v = a[sl].copy()
            if b == api.PLAN_GROUP:
                v = v - base
            elif b == api.PLAN_SAFETY:
                v["closest_agent"] = np.where(v["closest_agent"] >= 0, v["closest_agent"] - base, v["closest_agent"])
        out[b] = np.ascontiguousarray(v).tobytes()
    return out


def differ(a, b):
    return [k for k in a if a[k] != b[k]]


def fly(api, torch, plan, n, starts, goals, steps, graph, before=None):
    plan.reset(starts, goals)
    trace = []
    for _ in range(steps):
        if before is not None:
            before.append((plan.get(api.PLAN_PLAN).copy(), plan.get(api.PLAN_GOAL).copy()))
        plan.step(graph=graph)
        torch.cuda.synchronize()
        trace.append(snapshot(api, plan, n))
    return trace


def pair_specs(env, k, local):
    base = int(env["off"][k])
    return MC.straight_and_chaser(env["W"]["z_2d"], k, 0 if local else base)  # the chaser is after its mission's first agent


def give_pairs(api, env, plan, missions, local=False, shared=False):
    """Every mission of `missions` gets its pair (a straight obstacle, a chaser); local: agent ids of a plan of that mission alone;
    shared: all of them in ONE table (lscqp_plan_set_obstacles), which is what the parent offers."""
    specs = [pair_specs(env, k, local) for k in missions]
    flat = [s for per in specs for s in per]
    if shared:
        plan.set_obstacles(api.obstacle_models(flat))
    else:
        plan.set_mission_obstacles([api.obstacle_models(per) for per in specs])
    drives, history = api.obstacle_drives(flat, plan.n_total)
    plan.set_obstacle_drives(drives, history)


@pytest.fixture(scope="module", params=["LSC", "CLSC"])
def flown(request, api, torch_cuda, env):
    """Equal counts: the partition with a pair per mission through the graph, and every mission alone with lscqp_plan_set_obstacles."""
    mode = api.GEN_LSC if request.param == "LSC" else api.GEN_CLSC
    K = len(SIZES)
    plan = make_plan(api, env, mode, env["n"], env["off"])
    give_pairs(api, env, plan, range(K))
    whole = fly(api, torch_cuda, plan, env["n"], env["starts"], env["goals"], K_REPLANS, True)
    nodes = plan.graph_nodes()
    plan.close()
    singles = []
    for k, sl in enumerate(env["sl"]):
        one = make_plan(api, env, mode, SIZES[k])
        give_pairs(api, env, one, [k], local=True, shared=True)
        singles.append(fly(api, torch_cuda, one, SIZES[k], env["starts"][sl], env["goals"][sl], K_REPLANS, True))
        one.close()
    return dict(mode=mode, whole=whole, singles=singles, nodes=nodes)


def test_equal_counts_every_mission_flies_the_bytes_of_its_own_plan(api, env, flown):
    """All 19 plan buffers, the obstacle table, the safety buffer and the clock after every replan, slice by slice.  (Equal counts on
    purpose: with unequal ones a mission alone has another row layout and kernel instance, and bit identity is not promised.)"""
    moved = 0.0
    for k, sl in enumerate(env["sl"]):
        for r in range(K_REPLANS):
            got = mission_slice(api, flown["whole"][r], sl, int(env["off"][k]), slice(2 * k, 2 * k + 2), k)
            want = mission_slice(api, flown["singles"][k][r], slice(0, SIZES[k]), 0)
            assert not differ(got, want), (k, r, differ(got, want))
        first, last = flown["whole"][0]["table"][2 * k:2 * k + 2], flown["whole"][-1]["table"][2 * k:2 * k + 2]
        moved = np.abs(last["position"] - first["position"]).max(1).min()
        assert moved > 0.1, (k, moved)  # the straight one and the chaser both moved
    assert flown["whole"][-1]["clock"].tolist() == [K_REPLANS] * len(SIZES)
    fig = flown["whole"][-1]["obs_safety"]
    assert np.isfinite(fig["safety_ratio_obs"]).all() and set(fig["closest_obstacle"].tolist()) <= {0, 1}  # slots, not table indices
    tabs = [flown["whole"][-1]["table"][2 * k:2 * k + 2].tobytes() for k in range(len(SIZES))]
    assert len(set(tabs)) == len(SIZES)  # (no two missions have the same obstacles)


def test_eager_equals_graph_with_the_node_count_of_a_shared_table_of_as_many_slots(api, torch_cuda, env, flown):
    plan = make_plan(api, env, flown["mode"], env["n"], env["off"])
    give_pairs(api, env, plan, range(len(SIZES)))
    eager = fly(api, torch_cuda, plan, env["n"], env["starts"], env["goals"], K_REPLANS, False)
    assert plan.graph_nodes() == 0
    plan.close()
    for r in range(K_REPLANS):
        a, b = (mission_slice(api, t[r], slice(0, env["n"]), 0) for t in (eager, flown["whole"]))
        assert not differ(a, b), (r, differ(a, b))
    shared = make_plan(api, env, flown["mode"], env["n"], env["off"])
    give_pairs(api, env, shared, [0], shared=True)  # one shared table of two entries: two obstacle slots as well
    fly(api, torch_cuda, shared, env["n"], env["starts"], env["goals"], 2, True)
    assert flown["nodes"] == shared.graph_nodes() > 0
    shared.close()


@pytest.fixture(scope="module")
def unequal(api, torch_cuda, env, flown):
    """Counts (2, 0, 1) flown eagerly, with the plans and goals every replan started from; and the flight that differs in mission 0's
    models only."""
    z = env["W"]["z_2d"]
    out = {}
    for name, shift in (("base", 0.0), ("other", 0.75)):
        specs = MC.unequal_specs(z)
        for s in specs[0]:
            for key in ("start", "goal"):
                if key in s:
                    s[key] = [s[key][0], s[key][1] + shift, s[key][2]]
            if "waypoints" in s:
                s["waypoints"] = [[w[0], w[1] + shift, w[2]] for w in s["waypoints"]]
        plan = make_plan(api, env, flown["mode"], env["n"], env["off"])
        plan.set_mission_obstacles([api.obstacle_models(per) if per else None for per in specs])
        before = []
        out[name] = dict(trace=fly(api, torch_cuda, plan, env["n"], env["starts"], env["goals"], K_REPLANS, False, before), before=before)
        plan.close()
    return out


def test_unequal_counts_padded_slots_are_zero_rows_and_live_slots_the_generators(api, torch_cuda, env, flown, unequal):
    """Counts (2, 0, 1), n_slot = 2: slots 0, 1 of mission 1's agents and slot 1 of mission 2's hold all-zero rows at every replan; the live
    slots equal one lscqp_generate_obstacle_rows_device call on what the chain itself held (the table, headers, the goals and the shifted
    plans the replan started from), with the agents' own ids."""
    torch, sol, n, M = torch_cuda, env["sol"], env["n"], 10
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    ids = np.full((n, 2), -1, np.int32)
    ids[env["sl"][0]] = [0, 1]
    ids[env["sl"][2], 0] = 2
    par = api.ObstacleParam(1.0, 0.75, 3.0, 0.1, 1, 1)
    radius = np.full(n, env["W"]["radius"])
    live = 0.0
    for r, s in enumerate(unequal["base"]["trace"]):
        rows = s[api.PLAN_ROWS].view(np.float64).reshape(n, MC.N_OBS, M * 6 * 4)
        assert not rows[env["sl"][1], :2].any() and not rows[env["sl"][2], 1].any(), r
        assert s["table"].shape == (3,) and s["clock"].tolist() == [r + 1] * 3
        if r == 0:
            continue
        x_before, goal_before = unequal["base"]["before"][r]
        d_own = torch.zeros(n * M * 18, dtype=torch.float64, device=dev)
        sol.shift_traj_device(n, up(x_before).view(torch.float64), d_own, z_2d=env["W"]["z_2d"])
        d_rows = torch.full((n * MC.N_OBS * M * 6 * 4,), np.nan, dtype=torch.float64, device=dev)
        sol.generate_obstacle_rows_device(flown["mode"], par, n, 2, 0, d_own, up(ids), up(s["table"]), None, up(radius).view(torch.float64),
                                          up(goal_before).view(torch.float64), up(s[api.PLAN_HEADER]), d_rows, MC.N_OBS, 0)
        torch.cuda.synchronize()
        want = d_rows.cpu().numpy().reshape(n, MC.N_OBS, M * 6 * 4)
        assert want[:, :2].tobytes() == rows[:, :2].tobytes(), r
        live = max(live, float(np.abs(rows[env["sl"][0], :2]).max()), float(np.abs(rows[env["sl"][2], 0]).max()))
    assert live > 0


def test_unequal_counts_the_mission_without_obstacles_compares_nothing(api, env, unequal):
    for r, s in enumerate(unequal["base"]["trace"]):
        fig = s["obs_safety"]
        none = fig[env["sl"][1]]
        assert np.isposinf(none["safety_ratio_obs"]).all() and (none["closest_obstacle"] == -1).all() and (none["sample"] == -1).all(), r
        assert np.isfinite(fig[env["sl"][0]]["safety_ratio_obs"]).all() and np.isfinite(fig[env["sl"][2]]["safety_ratio_obs"]).all()
        assert (fig[env["sl"][2]]["closest_obstacle"] == 0).all() and set(fig[env["sl"][0]]["closest_obstacle"].tolist()) <= {0, 1}


def test_unequal_counts_other_models_in_mission_0_leave_missions_1_and_2_untouched(api, env, unequal):
    """The second flight differs in mission 0's models only: every buffer slice of missions 1 and 2, their table entry and their clocks
    are byte-identical at every replan -- and mission 0's are not."""
    changed = False
    for r in range(K_REPLANS):
        a, b = unequal["base"]["trace"][r], unequal["other"]["trace"][r]
        for k in (1, 2):
            sl, osl = env["sl"][k], slice(2, 2) if k == 1 else slice(2, 3)
            x, y = (mission_slice(api, t, sl, int(env["off"][k]), osl, k) for t in (a, b))
            assert not differ(x, y), (r, k, differ(x, y))
        x, y = (mission_slice(api, t, env["sl"][0], 0, slice(0, 2), 0) for t in (a, b))
        changed = changed or bool(differ(x, y))
    assert changed


def test_plan_run_keeps_the_obstacle_records_of_the_single_plans_at_either_check_every(api, torch_cuda, env, flown):
    """lscqp_plan_run with the obstacle record at check_every 1 and 16, with the threshold mission 0 meets at replan 12 of the flown
    flight: byte-identical records, and mission k's is the record of mission k alone (its agent a global id, its obstacle the slot)."""
    plane = env["goals"].copy()
    plane[:, 2] = float(np.float32(env["W"]["z_2d"]))
    p0 = flown["whole"][12][api.PLAN_HEADER].view(api.HEADER_DTYPE).reshape(-1)["p0"]
    thr = float(RR.vector3_distance(p0[env["sl"][0]], plane[env["sl"][0]]).max()) + 1e-3

    def records(plan, n, starts, goals):
        plan.set_record(thr)
        plan.set_obstacle_record()
        out = {}
        for every in (1, 16):
            plan.reset(starts, goals)
            plan.run(20, check_every=every)
            out[every] = (plan.record().download()[0].copy(),) + tuple(a.copy() for a in plan.record().obstacles())
        plan.close()
        for a, b in zip(out[1], out[16]):
            assert a.tobytes() == b.tobytes()
        return out[1]

    plan = make_plan(api, env, flown["mode"], env["n"], env["off"])
    give_pairs(api, env, plan, range(len(SIZES)))
    rec, ms, ag = records(plan, env["n"], env["starts"], env["goals"])
    assert rec["finished"][0] == 1 and rec["replans"][0] <= 13
    for k, sl in enumerate(env["sl"]):
        one = make_plan(api, env, flown["mode"], SIZES[k])
        give_pairs(api, env, one, [k], local=True, shared=True)
        rec1, ms1, ag1 = records(one, SIZES[k], env["starts"][sl], env["goals"][sl])
        want = ms1.copy()
        want["agent"] += int(env["off"][k])
        assert RC.same_structs(ms[k:k + 1], want) and RC.same_structs(ag[sl], ag1), k
        assert rec["replans"][k] == rec1["replans"][0] and rec["finished"][k] == rec1["finished"][0]
        assert np.isfinite(ms["safety_ratio_obs"][k]) and 0 <= ms["obstacle"][k] < 2


def test_two_missions_over_two_worlds_with_their_own_obstacles(api, torch_cuda, env, flown):
    """Worlds compose unchanged: missions of six and five agents over two fixture worlds, a pair of obstacles each, twelve replans -- every
    mission's slice is a plan of that mission alone over its own map with lscqp_plan_set_obstacles."""
    g = WLD.fixture()
    W = WLD.world(0, g)
    sizes = [6, 5]
    off, starts, goals = WLD.seeded_missions(sizes, seed=1, g=g)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    maps = [api.WorldMap(g["worlds"][k], W["world_min"], W["world_max"], W["resolution"], W["max_dist"]) for k in range(2)]
    e2 = dict(W=W, sol=sol, wmap=maps[0], off=off)
    n, steps = int(off[-1]), 12
    ws = api.Worlds(maps)
    plan = make_plan(api, e2, flown["mode"], n, off)
    plan.set_worlds(ws)
    give_pairs(api, e2, plan, range(2))
    whole = fly(api, torch_cuda, plan, n, starts, goals, steps, True)
    plan.close()
    ws.close()
    for k, sl in enumerate(WLD.slices(off)):
        one = make_plan(api, e2, flown["mode"], sizes[k], wmap=maps[k])
        give_pairs(api, e2, one, [k], local=True, shared=True)
        single = fly(api, torch_cuda, one, sizes[k], starts[sl], goals[sl], steps, True)
        one.close()
        for r in range(steps):
            got = mission_slice(api, whole[r], sl, int(off[k]), slice(2 * k, 2 * k + 2), k)
            want = mission_slice(api, single[r], slice(0, sizes[k]), 0)
            assert not differ(got, want), (k, r, differ(got, want))
    for m in maps:
        m.close()
    sol.close()


def test_the_lifecycle_and_every_refusal_with_its_cause(api, torch_cuda, env, flown):
    """A step before the reset is refused; the two setters replace each other; taking the obstacles away restores the plain chain's node
    count; each refusal names its cause and leaves the plan as it was."""
    torch, n, off = torch_cuda, env["n"], env["off"]
    K = len(SIZES)
    z = env["W"]["z_2d"]
    per = [api.obstacle_models(pair_specs(env, k, False)) for k in range(K)]
    bare = make_plan(api, env, flown["mode"], n, off)
    fly(api, torch, bare, n, env["starts"], env["goals"], 2, True)
    bare_nodes = bare.graph_nodes()
    bare.close()

    plan = make_plan(api, env, flown["mode"], n, off)
    # --- the count of the partition in force, at the call
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_mission_obstacles: 2 obstacle tables for 3 missions") as e:
        plan.set_mission_obstacles(per[:2])
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    # --- more obstacles in one mission than row slots
    with pytest.raises(api.LscqpError, match="a mission's obstacle count exceeds the plan's row slots per agent") as e:
        plan.set_mission_obstacles([np.concatenate([per[0]] * 4), per[1], per[2]])
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    # --- a model the preparation refuses
    bad = per[1].copy()
    bad["speed"][0] = 0.0
    with pytest.raises(api.LscqpError, match="model 2: speed <= 0"):
        plan.set_mission_obstacles([per[0], bad, per[2]])
    assert plan.obstacle_pointer(api.PLAN_OBS_TABLE) == (None, 0)
    plan.reset(env["starts"], env["goals"])
    plan.step(graph=True)  # (refused calls: the plan as it was, no reset asked for on their account)
    # --- the setter, and the step before the reset
    plan.set_mission_obstacles(per)
    for graph in (False, True):
        with pytest.raises(api.LscqpError, match="lscqp_plan_set_mission_obstacles: lscqp_plan_reset must come before the next step"):
            plan.step(graph=graph)
    assert plan.obstacle_pointer(api.PLAN_OBS_TABLE)[1] == 2 * K * api.OBSTACLE_DTYPE.itemsize
    assert plan.obstacle_pointer(api.PLAN_OBS_CLOCK)[1] == 4 * K and plan.obstacle_pointer(api.PLAN_OBS_SAFETY)[1] == n * api.SAFETY_OBS_DTYPE.itemsize
    # --- drives: the total, and a chaser after an agent of another mission
    flat = [s for k in range(K) for s in pair_specs(env, k, False)]
    drives, history = api.obstacle_drives(flat, n)
    with pytest.raises(api.LscqpError, match="n_dyn is not the number of the plan's obstacles"):
        plan.set_obstacle_drives(drives[:2], history)
    stray = drives.copy()
    stray["target_agent"][3] = 0  # mission 1's chaser after an agent of mission 0
    with pytest.raises(api.LscqpError, match="model 3: target_agent 0 lies outside mission 1, which owns the chaser") as e:
        plan.set_obstacle_drives(stray, history)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    plan.set_obstacle_drives(drives, history)
    # --- another mission count while these obstacles are set (the rule of the worlds); the same count with other offsets is taken
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_missions: the plan has 3 obstacle tables") as e:
        plan.set_missions([0, 5, n])
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_missions: the plan has 3 obstacle tables"):
        plan.set_missions(None)
    # --- the flight log, in either order
    plan.set_record(0.1)
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_flight_log: the plan has a table of obstacles per mission") as e:
        plan.set_flight_log(8)
    assert e.value.code == api.ERR_UNSUPPORTED
    plan.set_record(None)
    # --- it flies what the flown plan flew, with its node count (the refused calls changed nothing)
    got = fly(api, torch, plan, n, env["starts"], env["goals"], 4, True)
    for r in range(4):
        a, b = (mission_slice(api, t[r], slice(0, n), 0) for t in (got, flown["whole"]))
        assert not differ(a, b), (r, differ(a, b))
    assert plan.graph_nodes() == flown["nodes"]
    # --- the partition moved under the same count: every agent's list follows at the reset (agent 3 now sees mission 1's pair) ...
    plan.set_missions([0, 3, 7, n])
    plan.reset(env["starts"], env["goals"])
    plan.step()
    torch.cuda.synchronize()
    fig = plan.get_obstacles(api.PLAN_OBS_SAFETY)
    # ... and a partition that takes a chaser's target out of its mission is refused by the reset that finds it so
    plan.set_missions([0, 5, 7, n])
    with pytest.raises(api.LscqpError, match="model 3: target_agent 4 lies outside mission 1, which owns the chaser") as e:
        plan.reset(env["starts"], env["goals"])
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    plan.set_missions(off)
    # --- lscqp_plan_set_obstacles replaces the tables (one clock, one table for all), and the new setter replaces that again
    plan.set_obstacles(per[0])
    assert plan.obstacle_pointer(api.PLAN_OBS_CLOCK)[1] == 4 and plan.graph_nodes() == 0
    plan.set_mission_obstacles(per)
    assert plan.obstacle_pointer(api.PLAN_OBS_CLOCK)[1] == 4 * K
    plan.set_obstacle_drives(drives, history)
    got = fly(api, torch, plan, n, env["starts"], env["goals"], 3, True)
    for r in range(3):
        a, b = (mission_slice(api, t[r], slice(0, n), 0) for t in (got, flown["whole"]))
        assert not differ(a, b), (r, differ(a, b))
    # --- taken away: the plain chain's node count and no obstacle buffer (either way of saying it)
    plan.set_mission_obstacles(None)
    assert plan.graph_nodes() == 0 and plan.obstacle_pointer(api.PLAN_OBS_TABLE) == (None, 0)
    fly(api, torch, plan, n, env["starts"], env["goals"], 2, True)
    assert plan.graph_nodes() == bare_nodes
    plan.set_mission_obstacles(per)
    plan.set_mission_obstacles([None, None, None])
    assert plan.obstacle_pointer(api.PLAN_OBS_TABLE) == (None, 0)
    plan.step(graph=True)  # (nothing pending: the obstacles are gone, and with them the reset they asked for)
    assert np.isfinite(fig["safety_ratio_obs"]).all()
    plan.close()
    # --- a log first, then the tables
    logged = make_plan(api, env, flown["mode"], n, off)
    logged.set_record(0.1)
    logged.set_flight_log(8)
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_mission_obstacles: the plan has a flight log") as e:
        logged.set_mission_obstacles(per)
    assert e.value.code == api.ERR_UNSUPPORTED
    logged.close()
    # --- a plan without a partition takes one table (K = 1) and no more
    alone = make_plan(api, env, flown["mode"], SIZES[0])
    with pytest.raises(api.LscqpError, match="3 obstacle tables for 1 missions"):
        alone.set_mission_obstacles(per)
    alone.set_mission_obstacles(per[:1])
    alone.close()
    # --- a sharded plan, and a BVC plan
    W = env["W"]
    part = api.Plan(env["sol"], env["wmap"], 2, MC.N_OBS, WD.agents(api, W["radius"], 4), n_total=4, first_agent=0, constraint_mode=flown["mode"],
                    sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True, z_2d=z)
    with pytest.raises(api.LscqpError, match="a table per mission needs every agent on this device") as e:
        part.set_mission_obstacles(per[:1])
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    part.close()
    bvc = api.Plan(env["sol"], env["wmap"], 4, MC.N_OBS, WD.agents(api, W["radius"], 4), constraint_mode=api.GEN_BVC, sfc_mode=api.SFC_FROM_POINT, optimize_goal=False,
                   closed_loop=True, z_2d=z, prediction_mode=api.TRAJ_FROM_POSITION, initial_traj_mode=api.TRAJ_FROM_POSITION)
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_mission_obstacles: constraint_mode must be LSCQP_GEN_LSC") as e:
        bvc.set_mission_obstacles(per[:1])
    assert e.value.code == api.ERR_UNSUPPORTED
    bvc.close()


def test_closed_loop_tool_flies_each_mission_among_its_own_obstacles(api, torch_cuda, env):
    """tools/closed_loop.py with a list of obstacles per mission -- counts (2, 0, 2), the last mission's with a chaser after ITS agent 0, driven
    on the device: to the finish (six replans) it prints every mission's safety_ratio_obs from the obstacle record, stepped (four replans)
    from the buffer; the mission without obstacles reports +inf; the obstacles take two row slots, not four."""
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import closed_loop

    z = env["W"]["z_2d"]
    specs = [MC.unequal_specs(z)[0], [], MC.straight_and_chaser(z, 2, 0)]
    models = [api.obstacle_models(s) if s else None for s in specs]
    world = os.path.join(root, "tests", "golden", "forest10_world.json")
    log = closed_loop.run(world, missions=3, until_finished=6, mission_obstacles=models, mission_obstacle_specs=specs)
    per = log["per_mission"]
    assert [m["replans"] for m in per] == [6, 6, 6] and (log["obstacles"], log["obstacle_slots"], log["driven_obstacles"]) == (4, 2, 1)
    assert log["obstacles_per_mission"] is True and log["row_slots"] == 9 + 2
    assert np.isfinite(per[0]["safety_ratio_obs"]) and np.isposinf(per[1]["safety_ratio_obs"]) and np.isfinite(per[2]["safety_ratio_obs"])
    assert 0 <= per[0]["obstacle_safety_agent"] < 10 and 20 <= per[2]["obstacle_safety_agent"] < 30 and per[1]["obstacle_safety_obstacle"] == -1
    assert 0 <= per[2]["obstacle_safety_obstacle"] < 2  # the slot
    stepped = closed_loop.run(world, missions=3, steps=4, mission_obstacles=models, mission_obstacle_specs=specs)
    got = [m["safety_ratio_obs"] for m in stepped["per_mission"]]
    assert np.isfinite(got[0]) and np.isposinf(got[1]) and np.isfinite(got[2]) and stepped["min_obstacle_safety_ratio"] == min(got)
    with pytest.raises(ValueError, match="one list per mission"):
        closed_loop.run(world, missions=2, steps=1, mission_obstacles=models)
    with pytest.raises(ValueError, match="one shared table"):
        closed_loop.run(world, missions=3, until_finished=2, mission_obstacles=models, log_csv="unused")
