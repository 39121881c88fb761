"""Chasing and gaussian obstacles inside the replan chain (include/lscqp.h, "chasing and gaussian obstacles": lscqp_plan_set_obstacle_drives;
csrc/lscplan.hip, lscobstacle.hip).

The scenario is tests/test_obstacles_plan_gpu.py's -- the 3-D room, six agents on a ring, M = 5, LSC rows, closed loop -- with three
obstacles: that module's straight one, a chaser after agent 0 and a gaussian obstacle; n_obs = 8 row slots per agent (slots 0 .. 2 the
obstacles).  Twelve replans.  The flight to the finish (lscqp_plan_run needs the device's own waypoints) is forest10's 2-D mission with a
chaser and a gaussian obstacle.

One eager flight with drives is made once per module (`flown`), with every buffer of every replan kept; the tests read it and leave it
unchanged."""
import numpy as np
import pytest

from tests import obstacle_drive_reference as D
from tests import test_obstacles_plan_gpu as OP

pytestmark = pytest.mark.gpu

N, DT, K = OP.N, OP.DT, 12
N_DYN, N_OBS = 3, 8
CHASER, GAUSS = 1, 2


def obstacle_specs():
    return [OP.obstacle_specs()[0],
            dict(type="chasing", start=[-3.5, -3.5, 3.5], size=0.15, max_vel=0.3, max_acc=1.0, gamma_target=1.0, gamma_obs=1.0, downwash=1.0, target_agent=0),
            dict(type="gaussian", start=[3.5, -3.5, 0.5], size=0.15, initial_vel=[-0.1, 0.1, 0.0], max_vel=0.3, stddev_acc=0.5, max_acc=1.0,
                 acc_update_cycle=0.0, downwash=1.0)]


def make(api, env, drives=True, **kw):
    plan = OP.make_plan(api, env["sol"], env["wmap"], n_obs=N_OBS, **kw)
    plan.set_obstacles(env["models"], OP.obstacle_param(api))
    if drives:
        plan.set_obstacle_drives(env["drives"], env["history"])
    return plan


@pytest.fixture(scope="module")
def env(api, torch_cuda):
    W = OP.world()
    sol = OP.make_solver(api, W)
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    specs = obstacle_specs()
    drives, history = api.obstacle_drives(specs, N, horizon=K * DT, seed=1)
    yield dict(W=W, sol=sol, wmap=wmap, models=api.obstacle_models(specs), drives=drives, history=history)
    sol.close()


@pytest.fixture(scope="module")
def flown(api, torch_cuda, env):
    plan = make(api, env)
    snaps = OP.fly(api, torch_cuda, plan, env["W"]["starts"], env["W"]["goals"], K, graph=False)
    yield dict(plan=plan, snaps=snaps)
    plan.close()


def _differ(a, b):
    return [i for i in range(len(a)) if a[i] != b[i]]


def test_the_driven_plan_is_a_held_plan_whose_entries_the_host_writes_from_the_restatement(api, torch_cuda, env, flown):
    """(a) The twin has the same models without drives; before every replan the host downloads the state and the table, moves the chasing and
    the gaussian entry by the restatement and uploads the table.  Every plan and obstacle buffer of every replan is byte-identical."""
    W = env["W"]
    twin = make(api, env, drives=False)
    twin.reset(W["starts"], W["goals"])
    models = api.obstacle_model_prepare(env["models"])
    for r in range(K):
        table = twin.get_obstacles().copy()
        D.drive_table(models, env["drives"], env["history"], table, twin.get(api.PLAN_STATE).reshape(N, 9), r, DT)
        twin.put_obstacles(table)
        twin.step()
        torch_cuda.cuda.synchronize()
        got = OP.snapshot(api, twin)
        assert got == flown["snaps"][r], (r, _differ(got, flown["snaps"][r]))
    twin.close()
    first, last = (np.frombuffer(flown["snaps"][r][16 + api.PLAN_OBS_TABLE], api.OBSTACLE_DTYPE) for r in (0, K - 1))
    assert (first["position"][CHASER] == np.float32(env["models"]["start"][CHASER])).all()
    for i in (CHASER, GAUSS):  # both moved, the chaser towards agent 0
        assert np.abs(last["position"][i] - first["position"][i]).max() > 0.1
    p0 = np.frombuffer(flown["snaps"][K - 1][api.PLAN_HEADER], api.HEADER_DTYPE)["p0"][0]
    assert np.linalg.norm(last["position"][CHASER] - p0) < np.linalg.norm(first["position"][CHASER] - np.float32(W["starts"][0]))


def test_the_graph_replays_the_eager_chain_with_one_node_more_than_the_held_plan(api, torch_cuda, env, flown):
    """(b) ... and a plan with obstacles and no drives has the three nodes more than a plan without obstacles that it always had."""
    W = env["W"]
    plan = make(api, env)
    snaps = OP.fly(api, torch_cuda, plan, W["starts"], W["goals"], K, graph=True)
    for r in range(K):
        assert snaps[r] == flown["snaps"][r], (r, _differ(snaps[r], flown["snaps"][r]))
    held, bare = make(api, env, drives=False), OP.make_plan(api, env["sol"], env["wmap"], n_obs=N_OBS)
    for p in (held, bare):
        OP.fly(api, torch_cuda, p, W["starts"], W["goals"], 2, graph=True, keep=lambda *_: None)
    assert plan.graph_nodes() == held.graph_nodes() + 1 and held.graph_nodes() == bare.graph_nodes() + 3 and bare.graph_nodes() > 0
    for p in (plan, held, bare):
        p.close()


def test_the_setters_lifecycle(api, torch_cuda, env, flown):
    """(d) A step before the reset is refused; cleared drives, and drives dropped by a new lscqp_plan_set_obstacles, fly the HELD plan's bytes
    with its node count; a refused call leaves the plan as it was."""
    W = env["W"]
    held = make(api, env, drives=False)
    want = OP.fly(api, torch_cuda, held, W["starts"], W["goals"], 5, graph=True)
    held_nodes = held.graph_nodes()
    held.close()
    tab = np.frombuffer(want[-1][16 + api.PLAN_OBS_TABLE], api.OBSTACLE_DTYPE)
    assert (tab["position"][[CHASER, GAUSS]] == np.float32(env["models"]["start"][[CHASER, GAUSS]])).all()  # HELD at their start
    assert want[-1] != flown["snaps"][4]

    plan = OP.make_plan(api, env["sol"], env["wmap"], n_obs=N_OBS)
    with pytest.raises(api.LscqpError, match="the plan has no obstacles") as e:
        plan.set_obstacle_drives(env["drives"], env["history"])
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    plan.set_obstacles(env["models"], OP.obstacle_param(api))
    with pytest.raises(api.LscqpError, match="n_dyn is not the number of the plan's obstacles"):
        plan.set_obstacle_drives(env["drives"][:2], env["history"])
    plan.reset(W["starts"], W["goals"])
    plan.set_obstacle_drives(env["drives"], env["history"])
    for graph in (False, True):
        with pytest.raises(api.LscqpError, match="lscqp_plan_set_obstacle_drives: lscqp_plan_reset must come before the next step"):
            plan.step(graph=graph)
    snaps = OP.fly(api, torch_cuda, plan, W["starts"], W["goals"], 3, graph=True)
    assert all(snaps[r] == flown["snaps"][r] for r in range(3)) and plan.graph_nodes() == held_nodes + 1
    bad = env["drives"].copy()
    bad["target_agent"][CHASER] = N
    with pytest.raises(api.LscqpError, match="model 1: target_agent outside"):
        plan.set_obstacle_drives(bad, env["history"])
    bad = env["drives"].copy()
    bad["kind"][0] = api.DRIVE_CHASING
    with pytest.raises(api.LscqpError, match="model 0: a drive needs an LSCQP_OBSTACLE_HELD model"):
        plan.set_obstacle_drives(bad, env["history"])
    plan.step(graph=True)  # (refused calls: no reset asked for, the graph kept)
    torch_cuda.cuda.synchronize()
    assert OP.snapshot(api, plan) == flown["snaps"][3] and plan.graph_nodes() == held_nodes + 1
    # a second reset: the table back at the start, the checkpoints zeroed
    again = OP.fly(api, torch_cuda, plan, W["starts"], W["goals"], K, graph=True)
    assert all(again[r] == flown["snaps"][r] for r in range(K))
    # cleared drives
    plan.set_obstacle_drives(None)
    assert plan.graph_nodes() == 0
    got = OP.fly(api, torch_cuda, plan, W["starts"], W["goals"], 5, graph=True)
    assert got == want and plan.graph_nodes() == held_nodes
    # set_obstacles clears them as well
    plan.set_obstacle_drives(env["drives"], env["history"])
    plan.set_obstacles(env["models"], OP.obstacle_param(api))
    got = OP.fly(api, torch_cuda, plan, W["starts"], W["goals"], 5, graph=True)
    assert got == want and plan.graph_nodes() == held_nodes
    plan.close()


def test_two_missions_share_the_driven_obstacles_and_two_owners_equal_the_single_plan(api, torch_cuda, env, flown):
    """(e) As tests/test_obstacle_clsc_plan_gpu.py.  Two copies of the six agents as two missions of one plan: target_agent 0 is GLOBAL agent 0,
    which flies in mission 0 as it does alone, so the table and each mission's slice of every per-agent buffer are the single plan's.  Two
    owners of three agents each drive their own copy of the table from their own copy of the state buffer, exchanged after every replan."""
    W = env["W"]
    plan = make(api, env, n=2 * N, mission_offsets=[0, N, 2 * N])
    snaps = OP.fly(api, torch_cuda, plan, np.tile(W["starts"], (2, 1)), np.tile(W["goals"], (2, 1)), K, graph=True)
    plan.close()
    per_agent = [w for w in OP.PLAN_BUFFERS if w != api.PLAN_SAFETY] + [16 + api.PLAN_OBS_SAFETY]
    for r in range(K):
        for w in per_agent:
            one = flown["snaps"][r][w]
            assert snaps[r][w] == one + one, (r, w)
        assert snaps[r][16 + api.PLAN_OBS_TABLE] == flown["snaps"][r][16 + api.PLAN_OBS_TABLE], r
    h = N // 2
    parts = [make(api, env, n=h, n_total=N, first=f, safety=0) for f in (0, h)]
    for p in parts:
        p.reset(W["starts"], W["goals"])
    for r in range(K):
        for p in parts:
            p.step(graph=True)
        torch_cuda.cuda.synchronize()
        s = flown["snaps"][r]
        for w, per in ((api.PLAN_PLAN, OP.NV), (api.PLAN_STATE, 9), (api.PLAN_GOAL, 3)):
            full = [p.get(w).reshape(N, per) for p in parts]
            merged = np.concatenate([full[0][:h], full[1][h:]])
            assert merged.tobytes() == s[w], (r, w)
            for p in parts:
                p.put(w, merged)
        for w in (api.PLAN_ROWS, api.PLAN_STATUS, api.PLAN_OBJECTIVE):
            assert OP.raw(api, parts[0], w) + OP.raw(api, parts[1], w) == s[w], (r, w)
        for p in parts:
            assert OP.raw(api, p, api.PLAN_OBS_TABLE, obstacle=True) == s[16 + api.PLAN_OBS_TABLE], r
    for p in parts:
        p.close()


def test_a_flight_to_the_finish_logs_the_table_of_every_replan(api, torch_cuda):
    """(c) forest10 (2-D, the device's own waypoints) with a chaser after agent 0 and a gaussian obstacle, record and flight log.  A stepped
    flight tells the largest goal distance at the start of every replan and the table behind it; with the distance at replan 12 (plus a
    millimetre) as the threshold, lscqp_plan_run finishes the mission at the first replan that meets it, and the logged obstacle entries of
    every row are the stepped flight's table of that replan."""
    from tests import record_reference as RR
    from tests import waypoint_cases as WC
    from tests import waypoint_device as WD

    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    n, z = len(starts), W["z_2d"]
    specs = [dict(type="chasing", start=[4.8, 4.8, z], size=0.1, max_vel=0.3, max_acc=1.0, gamma_target=1.0, gamma_obs=1.0, downwash=1.0, target_agent=0),
             dict(type="gaussian", start=[-4.8, -4.8, z], size=0.1, initial_vel=[0.05, 0.05, 0.0], max_vel=0.2, max_acc=1.0, acc_update_cycle=0.1,
                  downwash=1.0, acc_history=np.c_[np.random.default_rng(2).normal(0.0, 0.3, (100, 2)), np.zeros(100)])]
    models = api.obstacle_models(specs)
    drives, history = api.obstacle_drives(specs, n)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    plan = api.Plan(sol, wmap, n, n - 1 + 2, WD.agents(api, W["radius"], n), constraint_mode=api.GEN_LSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True,
                    closed_loop=True, z_2d=z, safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT)
    plan.set_obstacles(models)
    plan.set_obstacle_drives(drives, history)
    plan.set_record(0.1)
    plan.reset(starts, goals)
    plane = goals.copy()
    plane[:, 2] = float(np.float32(z))
    far, tables = [], []
    for r in range(13):
        plan.step(graph=True)
        torch_cuda.cuda.synchronize()
        far.append(float(RR.vector3_distance(plan.get(api.PLAN_HEADER)["p0"], plane).max()))
        tables.append(plan.get_obstacles().copy())
    thr = far[12] + 1e-3
    first = min(r for r in range(13) if far[r] <= thr)
    plan.set_record(thr)
    plan.set_flight_log(40)
    plan.reset(starts, goals)
    enqueued = plan.run(40, check_every=4)
    rec, _ = plan.record().download()
    assert rec["finished"][0] == 1 and rec["replans"][0] == first + 1 and plan.record().unfinished() == 0 and enqueued == -(-(first + 1) // 4) * 4
    rows, over = plan.record().log_rows()
    assert rows.tolist() == [first + 1] and not over.any()
    _, _, logged = plan.record().log(0)
    assert logged.shape == (first + 1, 2, 4)
    for r in range(first + 1):
        want = np.c_[tables[r]["position"], tables[r]["radius"]].astype(np.float32)
        assert logged[r].tobytes() == want.tobytes(), r
    assert np.abs(tables[first]["position"] - tables[0]["position"]).max(1).min() > 0.02  # both obstacles moved
    assert (tables[first]["position"][:, 2] == np.float32(z)).all()                       # ... in the mission's plane
    plan.close()
    wmap.close()
    sol.close()
