"""The obstacle record inside a plan's chain (include/lscqp.h, "the obstacle record": lscqp_plan_set_obstacle_record): forest10's 2-D mission
on the device's own waypoints with two obstacles in its plane -- a straight one and a patrol, as tests/test_obstacles_plan_gpu.py builds
them -- LSC and CLSC rows.  The obstacle record is held to the plain-Python restatement (tests/record_obstacles_reference.py) fed with the
LSCQP_PLAN_OBS_SAFETY buffer a stepped twin held at every replan; then eager against graph, lscqp_plan_run at two check_every, two missions
against two single plans, the refusals and the setter's lifecycle."""
import numpy as np
import pytest

from tests import record_obstacles_cases as RC
from tests import record_obstacles_reference as ROR
from tests import record_reference as RR
from tests import waypoint_cases as WC
from tests import waypoint_device as WD

pytestmark = pytest.mark.gpu

K_REPLANS = 12
N_DYN = 2
PLAN_BUFFERS = range(19)  # LSCQP_PLAN_BUF_COUNT
OBS_BUFFERS = range(3)    # LSCQP_PLAN_OBS_COUNT


def specs(z):
    return [dict(type="straight", start=[2.0, -1.0, z], goal=[-2.0, 1.0, z], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0),
            dict(type="patrol", waypoints=[[-2.5, -1.5, z], [2.5, -1.5, z]], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0)]


def driven_specs(z):
    """tests/test_obstacle_drives_plan_gpu.py's chaser after agent 0 and gaussian obstacle."""
    return [dict(type="chasing", start=[4.8, 4.8, z], size=0.1, max_vel=0.3, max_acc=1.0, gamma_target=1.0, gamma_obs=1.0, downwash=1.0, target_agent=0),
            dict(type="gaussian", start=[-4.8, -4.8, z], size=0.1, initial_vel=[0.05, 0.05, 0.0], max_vel=0.2, max_acc=1.0, acc_update_cycle=0.1,
                 downwash=1.0, acc_history=np.c_[np.random.default_rng(2).normal(0.0, 0.3, (100, 2)), np.zeros(100)])]


@pytest.fixture(scope="module")
def env(api, torch_cuda):
    W = WC.forest10()
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    yield dict(W=W, sol=sol, wmap=wmap, starts=starts, goals=goals, n=len(starts), models=api.obstacle_models(specs(W["z_2d"])))
    wmap.close()
    sol.close()


def make_plan(api, env, mode, copies=1, obstacles=True, record=0.1):
    """forest10 (`copies` of it as missions of one plan) with n - 1 agent slots and two obstacle slots per agent."""
    W, n = env["W"], env["n"] * copies
    plan = api.Plan(env["sol"], env["wmap"], n, env["n"] - 1 + N_DYN, WD.agents(api, W["radius"], n), constraint_mode=mode, sfc_mode=api.SFC_FROM_HULL,
                    optimize_goal=True, closed_loop=True, z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT,
                    mission_offsets=None if copies == 1 else [env["n"] * c for c in range(copies + 1)])
    if obstacles:
        plan.set_obstacles(env["models"])
    if record is not None:
        plan.set_record(record)
    return plan


def raw(api, plan, which, obstacle=False):
    ptr, nb = plan.obstacle_pointer(which) if obstacle else plan.pointer(which)
    out = np.zeros(nb, np.uint8)
    if nb:
        api._call("lscqp_plan_obstacle_download" if obstacle else "lscqp_plan_download", plan._p, which, out, 0, nb)
    return out.tobytes()


def snapshot(api, plan):
    """Every plan buffer, every obstacle buffer, and the record's structs, distances and points."""
    out = [raw(api, plan, w) for w in PLAN_BUFFERS] + [raw(api, plan, w, obstacle=True) for w in OBS_BUFFERS]
    rec = plan.record()
    if rec is not None:
        m, d = rec.download()
        out += [m.tobytes(), d.tobytes(), rec.points().tobytes()]
    return out


def fly(api, torch, plan, env, k, graph, copies=1, keep=None):
    plan.reset(np.tile(env["starts"], (copies, 1)), np.tile(env["goals"], (copies, 1)))
    out = []
    for _ in range(k):
        plan.step(graph=graph)
        torch.cuda.synchronize()
        if keep is not None:
            out.append(keep(api, plan))
    return out


def stepped(api, torch, plan, env, k, copies=1):
    """A stepped flight of a plan WITHOUT the option: per replan the record's words before it and the LSCQP_PLAN_OBS_SAFETY buffer behind
    it -> the restated obstacle record after every replan, and the snapshots."""
    plan.reset(np.tile(env["starts"], (copies, 1)), np.tile(env["goals"], (copies, 1)))
    offsets = plan.missions()
    missions, agents = ROR.cleared(offsets)
    restated, snaps, least = [], [], []
    for _ in range(k):
        before, _ = plan.record().download()
        plan.step(graph=True)
        torch.cuda.synchronize()
        fig = plan.get_obstacles(api.PLAN_OBS_SAFETY)
        ROR.accumulate(missions, agents, offsets, RC.triples(fig), before["finished"], before["replans"])
        restated.append(ROR.as_arrays(np, api.MISSION_OBSTACLE_RECORD_DTYPE, api.AGENT_OBSTACLE_RECORD_DTYPE, missions, agents))
        snaps.append(snapshot(api, plan))
        least.append(float(fig["safety_ratio_obs"].min()))
    return restated, snaps, least


@pytest.fixture(scope="module", params=["LSC", "CLSC"])
def flown(request, api, torch_cuda, env):
    """The stepped twin of either constraint mode, flown once; the tests read it and leave it unchanged."""
    mode = api.GEN_LSC if request.param == "LSC" else api.GEN_CLSC
    twin = make_plan(api, env, mode)
    restated, snaps, least = stepped(api, torch_cuda, twin, env, K_REPLANS)
    nodes = twin.graph_nodes()
    twin.close()
    return dict(mode=mode, restated=restated, snaps=snaps, least=least, nodes=nodes)


def test_eager_and_graph_equal_the_restatement_with_one_node_more(api, torch_cuda, env, flown):
    """Twelve replans, eagerly and through the graph, with the option on: after every replan the obstacle record equals the restatement of
    the twin's LSCQP_PLAN_OBS_SAFETY, field for field; every plan buffer, obstacle buffer and the record's own bytes equal the twin's -- the
    option changes nothing else; and the graph has exactly one node more than the twin's.  The mission's figure is the least ratio of
    the flight and its replan the first that attains it."""
    for graph in (False, True):
        plan = make_plan(api, env, flown["mode"])
        plan.set_obstacle_record()

        def keep(api_, p):
            return snapshot(api_, p), p.record().obstacles()

        got = fly(api, torch_cuda, plan, env, K_REPLANS, graph, keep=keep)
        for r, (snap, (ms, ag)) in enumerate(got):
            assert RC.same_structs(ms, flown["restated"][r][0]) and RC.same_structs(ag, flown["restated"][r][1]), (graph, r)
            assert snap == flown["snaps"][r], (graph, r, [i for i in range(len(snap)) if snap[i] != flown["snaps"][r][i]])
        assert plan.graph_nodes() == (flown["nodes"] + 1 if graph else 0) and flown["nodes"] > 0
        plan.close()
    ms, ag = got[-1][1]
    least = flown["least"]
    assert np.isfinite(ms["safety_ratio_obs"][0]) and ms["safety_ratio_obs"][0] == min(least) and ms["replan"][0] == least.index(min(least))
    assert ms["compared"][0] == K_REPLANS * env["n"] and 0 <= ms["agent"][0] < env["n"] and 0 <= ms["obstacle"][0] < N_DYN
    assert ag["safety_ratio_obs"].min() == ms["safety_ratio_obs"][0] and ag["replan"][ms["agent"][0]] == ms["replan"][0]
    assert len(set(ag["replan"].tolist())) > 1  # (the agents' minima fall on different replans: the figures moved)


def test_two_missions_in_one_plan_are_two_single_plans(api, torch_cuda, env, flown):
    """Two copies of forest10 as two missions of one plan, the obstacles shared: each mission's obstacle record is the single plan's, the
    second one's agent shifted by the ten agents in front of it (a GLOBAL id); the agents' entries are the single plan's twice."""
    plan = make_plan(api, env, flown["mode"], copies=2)
    plan.set_obstacle_record()
    fly(api, torch_cuda, plan, env, K_REPLANS, True, copies=2)
    ms, ag = plan.record().obstacles()
    plan.close()
    one_m, one_a = flown["restated"][-1]
    want = np.concatenate([one_m, one_m])
    want["agent"][1] += env["n"]
    assert RC.same_structs(ms, want) and RC.same_structs(ag, np.concatenate([one_a, one_a]))
    assert ms["agent"][1] >= env["n"]


def test_plan_run_does_not_depend_on_check_every(api, torch_cuda, env, flown):
    """Driven obstacles (a chaser and a gaussian one), a flight log and the obstacle record, flown by lscqp_plan_run at check_every 1 and
    16 with the threshold the mission meets at replan 12 of a stepped flight: the mission freezes there, both runs give byte-identical
    obstacle records, and they are the restatement of the stepped flight's figures up to the freeze (the replans enqueued behind it
    changed nothing)."""
    W, n = env["W"], env["n"]
    dspecs = driven_specs(W["z_2d"])
    drives, history = api.obstacle_drives(dspecs, n)
    plan = make_plan(api, env, flown["mode"], obstacles=False, record=None)
    plan.set_obstacles(api.obstacle_models(dspecs))
    plan.set_obstacle_drives(drives, history)
    plan.set_record(0.1)
    plane = env["goals"].copy()
    plane[:, 2] = float(np.float32(W["z_2d"]))
    plan.reset(env["starts"], env["goals"])
    far, figs = [], []
    for r in range(13):
        plan.step(graph=True)
        torch_cuda.cuda.synchronize()
        far.append(float(RR.vector3_distance(plan.get(api.PLAN_HEADER)["p0"], plane).max()))
        figs.append(plan.get_obstacles(api.PLAN_OBS_SAFETY).copy())
    thr = far[12] + 1e-3
    first = min(r for r in range(13) if far[r] <= thr)
    missions, agents = ROR.cleared([0, n])
    for r in range(first + 1):
        ROR.accumulate(missions, agents, [0, n], RC.triples(figs[r]), [0], [r])
    want = ROR.as_arrays(np, api.MISSION_OBSTACLE_RECORD_DTYPE, api.AGENT_OBSTACLE_RECORD_DTYPE, missions, agents)
    plan.set_record(thr)
    plan.set_flight_log(40)
    plan.set_obstacle_record()
    out = {}
    for every in (1, 16):
        plan.reset(env["starts"], env["goals"])
        enqueued = plan.run(40, check_every=every)
        rec, _ = plan.record().download()
        assert rec["finished"][0] == 1 and rec["replans"][0] == first + 1 and enqueued == -(-(first + 1) // every) * every
        assert plan.record().log_rows()[0].tolist() == [first + 1]
        out[every] = plan.record().obstacles()
    plan.close()
    for a, b in zip(out[1], out[16]):
        assert a.tobytes() == b.tobytes()
    assert RC.same_structs(out[1][0], want[0]) and RC.same_structs(out[1][1], want[1])
    assert np.isfinite(want[0]["safety_ratio_obs"][0]) and want[0]["compared"][0] == (first + 1) * n


def test_the_refusals_each_named(api, torch_cuda, env, flown):
    plan = make_plan(api, env, flown["mode"], obstacles=False, record=None)
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_obstacle_record: the plan has no record \\(lscqp_plan_set_record first\\)") as e:
        plan.set_obstacle_record()
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    plan.set_obstacle_record(False)  # (nothing to take away: accepted)
    plan.set_record(0.1)
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_obstacle_record: the plan has no obstacles \\(lscqp_plan_set_obstacles first\\)") as e:
        plan.set_obstacle_record()
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    plan.set_obstacles(env["models"])
    plan.reset(env["starts"], env["goals"])
    plan.step(graph=True)  # (the refused calls changed nothing: no reset was asked for on their account)
    with pytest.raises(api.LscqpError, match="keeps no obstacle figures"):
        plan.record().obstacles()
    plan.set_obstacle_record()
    for graph in (False, True):
        with pytest.raises(api.LscqpError, match="lscqp_plan_set_obstacle_record: lscqp_plan_reset must come before the next step"):
            plan.step(graph=graph)
    plan.set_obstacle_record(False)  # (taken back: the plan may step again, as the plan it was)
    plan.step(graph=True)
    torch_cuda.cuda.synchronize()
    assert plan.record().download()[0]["replans"].tolist() == [2]
    plan.close()


def test_the_lifecycle_ends_in_the_bytes_of_the_final_configuration(api, torch_cuda, env, flown):
    """Set, clear, the record taken away, the obstacles taken away, a partition set and dropped, the flight log before and after, resets
    and replans in between: a plan that saw all of it flies the bytes -- buffers, record, flight log, obstacle record -- of a plan that only
    saw the final configuration, and the option switched off again gives the twin's bytes and node count back."""
    torch, n = torch_cuda, env["n"]

    def keep(api_, p):
        rec = p.record()
        return snapshot(api_, p), rec.obstacles(), [x.tobytes() for x in rec.log(0)]

    fresh = make_plan(api, env, flown["mode"])
    fresh.set_flight_log(K_REPLANS)
    fresh.set_obstacle_record()
    want = fly(api, torch, fresh, env, 10, True, keep=keep)
    fresh_nodes = fresh.graph_nodes()
    fresh.close()
    assert fresh_nodes == flown["nodes"] + 2  # (the log's node and the obstacle record's)

    plan = make_plan(api, env, flown["mode"])
    plan.set_obstacle_record()
    fly(api, torch, plan, env, 3, True)
    assert plan.graph_nodes() == flown["nodes"] + 1
    plan.set_obstacle_record(False)  # cleared
    assert plan.graph_nodes() == 0
    with pytest.raises(api.LscqpError, match="keeps no obstacle figures"):
        plan.record().obstacles()
    got = fly(api, torch, plan, env, 4, True, keep=snapshot)
    assert got == flown["snaps"][:4] and plan.graph_nodes() == flown["nodes"]  # (a plan that never heard of it)
    plan.set_obstacle_record()
    plan.set_record(None)  # the record taken away: the option with it
    plan.set_record(0.1)
    fly(api, torch, plan, env, 2, True)
    assert plan.graph_nodes() == flown["nodes"]
    with pytest.raises(api.LscqpError, match="keeps no obstacle figures"):
        plan.record().obstacles()
    plan.set_obstacle_record()
    plan.set_obstacles(None)  # the obstacles taken away: the option with them, and no reset is waited for on its account
    with pytest.raises(api.LscqpError, match="keeps no obstacle figures"):
        plan.record().obstacles()
    plan.reset(env["starts"], env["goals"])
    plan.step(graph=True)
    plan.set_obstacles(env["models"])
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_obstacles: lscqp_plan_reset must come before the next step"):
        plan.step()
    plan.set_obstacle_record()  # before the flight log ...
    plan.set_flight_log(K_REPLANS)
    plan.set_missions([0, 4, n])  # a partition: the record is made again at the reset, with the figures
    plan.reset(env["starts"], env["goals"])
    plan.step(graph=True)
    ms, ag = plan.record().obstacles()
    assert len(ms) == 2 and ms["replan"].tolist() == [0, 0] and 0 <= ms["agent"][0] < 4 <= ms["agent"][1] < n and ag["replan"].tolist() == [0] * n
    plan.set_missions(None)
    plan.set_obstacles(env["models"])  # new obstacles under a set option: the figures follow the new buffer
    plan.set_flight_log(0)
    plan.set_flight_log(K_REPLANS)  # ... and after it
    got = fly(api, torch, plan, env, 10, True, keep=keep)
    assert plan.graph_nodes() == fresh_nodes
    for r in range(10):
        assert got[r][0] == want[r][0], (r, [i for i in range(len(got[r][0])) if got[r][0][i] != want[r][0][i]])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[r][1], want[r][1])) and got[r][2] == want[r][2], r
        assert RC.same_structs(got[r][1][0], flown["restated"][r][0]) and RC.same_structs(got[r][1][1], flown["restated"][r][1]), r
    plan.close()


def test_closed_loop_tool_prints_every_missions_obstacle_figures(api, torch_cuda):
    """tools/closed_loop.py missions=2, until_finished=6 with the two obstacles: per mission the obstacle record's figure with its replan,
    GLOBAL agent and obstacle, and below_one, beside the keys it always printed; the flight's least figure is the smaller of the two."""
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import closed_loop

    world = os.path.join(root, "tests", "golden", "forest10_world.json")
    log = closed_loop.run(world, missions=2, until_finished=6, obstacles=api.obstacle_models(specs(WC.forest10()["z_2d"])))
    per = log["per_mission"]
    assert [m["replans"] for m in per] == [6, 6] and log["obstacles"] == 2 and "last_obstacle_safety_ratio" in log
    for k, m in enumerate(per):
        assert np.isfinite(m["obstacle_safety_ratio"]) and 0 <= m["obstacle_safety_replan"] < 6 and 0 <= m["obstacle_safety_obstacle"] < 2
        assert 10 * k <= m["obstacle_safety_agent"] < 10 * (k + 1) and m["below_one"] >= 0 and "min_safety_ratio" in m
    assert log["min_obstacle_safety_ratio"] == min(m["obstacle_safety_ratio"] for m in per) <= log["last_obstacle_safety_ratio"]
