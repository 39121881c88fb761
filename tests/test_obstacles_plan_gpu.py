"""Dynamic obstacles inside the replan chain (include/lscqp.h, "dynamic obstacles in the chain"; csrc/lscplan.hip, lscobstacle.hip).

The scenario: a 3-D room, six agents swapping sides of a ring (M = 5, LSC rows, corridors from constructSFCFromPoint, static goals, closed
loop, safety figures over two samples), two obstacles -- a straight one and a patrol, each across an agent's
path -- and n_obs = 7 row slots per agent: slots 0, 1 the obstacles, slots 2 .. 6 the five other agents.  Thirty replans.

One eager flight is made once per module (`flown`), with every buffer of every replan kept; the tests read it and leave it unchanged."""
import numpy as np
import pytest

from tests import obstacle_reference as R

pytestmark = pytest.mark.gpu

N, M, DIM, DT = 6, 5, 3, 0.2
N_DYN, N_OBS, K = 2, 7, 30
NV = DIM * M * 6
RADIUS, DOWNWASH = 0.15, 2.0
RESOLVE_AT = (3, 14, 25)


def world():
    """An 8 x 8 x 4 m room with four boxes, the agents on a tilted ring of 3 m radius, goals antipodal."""
    ang = np.linspace(0, 2 * np.pi, N, endpoint=False)
    starts = np.c_[3.0 * np.cos(ang), 3.0 * np.sin(ang), 2.0 + 0.8 * np.sin(2 * ang)]
    starts = np.round(starts * 4) / 4
    goals = np.c_[-starts[:, 0], -starts[:, 1], 4.0 - starts[:, 2]]
    boxes = [[1.5, -1.0, 2.75, 0.5, 0.5, 1.5], [-1.5, 1.25, 0.75, 0.5, 0.5, 1.5], [0.0, 2.0, 2.0, 0.8, 0.4, 0.6], [0.5, -2.25, 2.5, 0.4, 0.8, 0.5]]
    return dict(boxes=boxes, world_min=[-4.0, -4.0, 0.0], world_max=[4.0, 4.0, 4.0], resolution=0.1, max_dist=1.0, starts=starts, goals=goals)


def obstacle_specs():
    """Mission-file entries, chosen on the device (NOTES.md section 32) so that the flight has the four properties the first test asserts: the
    straight obstacle crosses the path of agent 0 (x = 1.5) while it flies by, the patrol goes to and fro across the path of agent 3.  Slow,
    small obstacles away from the middle of the ring, where the six agents meet anyway: faster or larger ones, or ones through the
    middle, leave some agent's QP INFEASIBLE at some replan (the oracle agrees) -- the rows are hard rows."""
    return [dict(type="straight", start=[1.5, -0.5, 2.0], goal=[1.5, 1.5, 2.0], size=0.2, speed=0.2, max_acc=1.0, downwash=1.0),
            dict(type="patrol", waypoints=[[-1.2, -0.6, 2.0], [-1.2, 0.6, 2.0]], size=0.2, speed=0.2, max_acc=1.0, downwash=1.0)]


def obstacle_param(api):
    """src/param.cpp:63-67, 106-108 at the launch files' values."""
    return api.ObstacleParam(1.0, 0.75, 3.0, 0.1, 1, 1)


def agents(api, n):
    ag = np.zeros(n, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = RADIUS, DOWNWASH, 1.0, 2.0, 1.0
    return ag


def make_solver(api, W):
    return api.Solver(api.make_desc(M=M, dim=DIM, dt=DT, comm_range=0.0, use_sfc=True, world_min=W["world_min"], world_max=W["world_max"]))


def make_plan(api, sol, wmap, n_obs=N_OBS, n=N, n_total=None, first=0, safety=2, mission_offsets=None):
    return api.Plan(sol, wmap, n, n_obs, agents(api, n if n_total is None else n_total), n_total=n_total, first_agent=first, constraint_mode=api.GEN_LSC,
                    sfc_mode=api.SFC_FROM_POINT, optimize_goal=False, closed_loop=True, safety_samples=safety, record_time_step=0.1,
                    mission_offsets=mission_offsets)


PLAN_BUFFERS = range(16)
OBS_BUFFERS = range(3)


def raw(api, plan, which, obstacle=False):
    """The bytes of one buffer of the plan (b"" where the plan has no such buffer)."""
    ptr, nb = plan.obstacle_pointer(which) if obstacle else plan.pointer(which)
    out = np.zeros(nb, np.uint8)
    if nb:
        api._call("lscqp_plan_obstacle_download" if obstacle else "lscqp_plan_download", plan._p, which, out, 0, nb)
    return out.tobytes()


def snapshot(api, plan):
    return [raw(api, plan, w) for w in PLAN_BUFFERS] + [raw(api, plan, w, obstacle=True) for w in OBS_BUFFERS]


def fly(api, torch, plan, starts, goals, k, graph, keep=snapshot):
    plan.reset(starts, goals)
    out = []
    for _ in range(k):
        plan.step(graph=graph)
        torch.cuda.synchronize()
        out.append(keep(api, plan))
    return out


def obstacle_slack(api, rows, x, status):
    """n . x - b of every obstacle-slot row at the control point it binds, [n][N_DYN][M][6]; +inf for agents whose QP is not OPTIMAL."""
    r = np.frombuffer(rows, api.ROW_DTYPE).reshape(-1, N_OBS, M, 6)[:, :N_DYN]
    p = np.frombuffer(x, np.float64).reshape(-1, DIM, M, 6)
    s = r["nx"] * p[:, None, 0] + r["ny"] * p[:, None, 1] + r["nz"] * p[:, None, 2] - r["b"]
    s[np.frombuffer(status, np.int32) != 0] = np.inf
    s[:, :, 0, :3] = np.inf  # (the QP holds no LSC row on the control points the initial state fixes, src/traj_optimizer.cpp:404-406)
    return s


@pytest.fixture(scope="module")
def env(api, torch_cuda):
    W = world()
    sol = make_solver(api, W)
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    raw_models = api.obstacle_models(obstacle_specs())
    yield dict(W=W, sol=sol, wmap=wmap, models=raw_models, objs=[R.from_model(m) for m in raw_models])
    sol.close()


@pytest.fixture(scope="module")
def flown(api, torch_cuda, env):
    """The scenario flown eagerly: per replan the plans BEFORE the step and every buffer after it.  And its twin without obstacles (n_obs = 7)."""
    W = env["W"]
    plan = make_plan(api, env["sol"], env["wmap"])
    plan.set_obstacles(env["models"], obstacle_param(api))
    before = []

    def keep(api_, p):
        return snapshot(api_, p)

    plan.reset(W["starts"], W["goals"])
    snaps = []
    for _ in range(K):
        before.append(raw(api, plan, api.PLAN_PLAN))
        plan.step()
        torch_cuda.cuda.synchronize()
        snaps.append(keep(api, plan))
    twin = make_plan(api, env["sol"], env["wmap"])
    twin_snaps = fly(api, torch_cuda, twin, W["starts"], W["goals"], K, graph=False)
    twin.step(graph=True)
    twin_nodes = twin.graph_nodes()
    twin.close()
    yield dict(plan=plan, snaps=snaps, before=before, twin=twin_snaps, twin_nodes=twin_nodes)
    plan.close()


def _table(api, snap):
    return np.frombuffer(snap[16 + api.PLAN_OBS_TABLE], api.OBSTACLE_DTYPE)


def test_every_qp_solves_and_the_obstacle_rows_keep_the_agents_away(api, oracle, env, flown):
    """Every QP OPTIMAL and valid; at least one obstacle-slot row active at a returned optimum; the obstacle safety ratio never below
    1 - 5e-6 (tests/test_plan.py's bar for float32 plans); and the same mission without obstacles, judged against the same obstacle
    positions, does come too close: the rows, not luck, kept the agents away."""
    W = env["W"]
    cls = oracle.make_class(M=M, dim=DIM, use_sfc=True, comm_range=0.0, world_min=W["world_min"], world_max=W["world_max"])
    min_slack, worst, worst_twin = np.inf, np.inf, np.inf
    for k, (s, t) in enumerate(zip(flown["snaps"], flown["twin"])):
        st = np.frombuffer(s[api.PLAN_STATUS], np.int32)
        assert (st == 0).all() and (np.frombuffer(s[api.PLAN_VALID], np.int32) == 1).all(), (k, st)
        assert (np.frombuffer(t[api.PLAN_STATUS], np.int32) == 0).all(), k
        min_slack = min(min_slack, float(obstacle_slack(api, s[api.PLAN_ROWS], s[api.PLAN_PLAN], s[api.PLAN_STATUS]).min()))
        worst = min(worst, float(np.frombuffer(s[16 + api.PLAN_OBS_SAFETY], api.SAFETY_OBS_DTYPE)["safety_ratio_obs"].min()))
        tab = _table(api, s)
        x_twin = np.frombuffer(t[api.PLAN_PLAN], np.float64).reshape(N, NV)
        worst_twin = min(worst_twin, float(oracle.safety_obstacles(cls, N, x_twin, RADIUS, DOWNWASH, np.c_[tab["position"], tab["radius"], tab["downwash"]],
                                                                     2, 0.1)[:, 0].min()))
    print("obstacle rows: least slack %.3e m; obstacle safety ratio %.6f with the rows, %.6f without" % (min_slack, worst, worst_twin))
    assert min_slack <= 1e-6, min_slack
    assert worst >= 1.0 - 5e-6, worst
    assert worst_twin < 1.0, worst_twin


def test_the_table_is_the_restatements_at_every_replans_clock(api, env, flown):
    """Replan r reads the obstacles at clock r: straight obstacles and the patrol's first lap bit for bit, later laps within one float32
    ulp of the coordinate and of `speed` (tests/test_obstacles_gpu.py says why); the clock word reads r + 1 behind replan r."""
    lap = [o.lap_time() if isinstance(o, R.Patrol) else np.inf for o in env["objs"]]
    for r, s in enumerate(flown["snaps"]):
        assert np.frombuffer(s[16 + api.PLAN_OBS_CLOCK], np.int32)[0] == r + 1
        tab, t = _table(api, s), R.clock_time(r, DT)
        for i, o in enumerate(env["objs"]):
            p, v = o.at(t)
            if t < lap[i]:
                assert np.array_equal(tab["position"][i], p.astype(np.float64)) and np.array_equal(tab["velocity"][i], v.astype(np.float64)), (r, i)
            else:
                assert (np.abs(tab["position"][i] - p) <= np.spacing(np.abs(p))).all(), (r, i)
                assert (np.abs(tab["velocity"][i] - v) <= np.spacing(np.float32(env["models"]["speed"][i]))).all(), (r, i)
            assert (tab["radius"][i], tab["downwash"][i], tab["max_acc"][i], tab["type"][i]) == (o.radius, o.downwash, o.max_acc, 0)


def test_the_obstacle_slots_are_the_standalone_generators_rows(api, torch_cuda, env, flown):
    """Slots [0, n_dyn) of LSCQP_PLAN_BUF_ROWS equal, bit for bit, one lscqp_generate_lsc_obstacles_device call on what the chain itself held:
    the table, headers and goals downloaded, the planning agents' initial trajectories rebuilt from the previous plans (the whole-segment
    shift, lscqp_shift_traj_device; on the first replan the agents hover: Trajectory::planConstVelTraj with zero velocity)."""
    torch, sol = torch_cuda, env["sol"]
    dev = torch.device("cuda", 0)
    up = lambda b, dt=np.uint8: torch.from_numpy(np.frombuffer(b, dt).copy()).to(dev)  # noqa: E731
    par = obstacle_param(api)
    d_ids = torch.from_numpy(np.tile(np.arange(N_DYN, dtype=np.int32), N)).to(dev)
    d_radius = torch.full((N,), RADIUS, dtype=torch.float64, device=dev)
    for k, s in enumerate(flown["snaps"]):
        if k == 0:
            p0 = np.float32(env["W"]["starts"]).astype(np.float64)
            own = np.broadcast_to(p0[:, None, None, :], (N, M, 6, 3)).copy()
            d_own = torch.from_numpy(own.reshape(-1)).to(dev)
        else:
            d_own = torch.zeros(N * M * 18, dtype=torch.float64, device=dev)
            sol.shift_traj_device(N, up(flown["before"][k], np.float64), d_own)
        d_rows = torch.full((N * N_OBS * M * 6 * 4,), np.nan, dtype=torch.float64, device=dev)
        sol.generate_lsc_obstacles_device(par, N, N_DYN, 0, d_own, d_ids, up(s[16 + api.PLAN_OBS_TABLE]), d_radius, up(s[api.PLAN_GOAL], np.float64),
                                          up(s[api.PLAN_HEADER]), d_rows, N_OBS, 0)
        torch.cuda.synchronize()
        want = d_rows.cpu().numpy().reshape(N, N_OBS, M * 6 * 4)
        got = np.frombuffer(s[api.PLAN_ROWS], np.float64).reshape(N, N_OBS, M * 6 * 4)
        assert np.isnan(want[:, N_DYN:]).all()  # (the call wrote its own slots only)
        assert want[:, :N_DYN].tobytes() == got[:, :N_DYN].tobytes(), k
        assert np.abs(got[:, :N_DYN]).max() > 0


def test_on_the_first_replan_the_agent_slots_are_a_plan_of_five_slots_without_obstacles(api, torch_cuda, env, flown):
    W = env["W"]
    twin = make_plan(api, env["sol"], env["wmap"], n_obs=N_OBS - N_DYN)
    t = fly(api, torch_cuda, twin, W["starts"], W["goals"], 1, graph=False)[0]
    twin.close()
    s = flown["snaps"][0]
    got = np.frombuffer(s[api.PLAN_ROWS], np.float64).reshape(N, N_OBS, -1)[:, N_DYN:]
    want = np.frombuffer(t[api.PLAN_ROWS], np.float64).reshape(N, N_OBS - N_DYN, -1)
    assert got.tobytes() == want.tobytes() and np.abs(want).max() > 0
    assert s[api.PLAN_IN_RANGE] == t[api.PLAN_IN_RANGE] and (np.frombuffer(s[api.PLAN_IN_RANGE], np.int32) == N - 1).all()
    assert (np.frombuffer(s[api.PLAN_HEADER], api.HEADER_DTYPE)["n_obs"] == N_OBS).all()


def test_three_replans_are_resolved_by_the_oracle_from_the_chains_buffers(api, oracle, env, flown):
    """Objective to 1e-8 relative, x as tests/test_plan.py: test_plan_chain_in_three_dimensions_with_static_goals holds it (2e-6 m; a flagged
    or flat-valley point 5e-5 m with its KKT residuals at 1e-8)."""
    from tests import helpers as H

    W = env["W"]
    cls = oracle.make_class(M=M, dim=DIM, use_sfc=True, comm_range=0.0, world_min=W["world_min"], world_max=W["world_max"])
    for k in RESOLVE_AT:
        s = flown["snaps"][k]
        hdr = np.frombuffer(s[api.PLAN_HEADER], api.HEADER_DTYPE)
        rows = np.frombuffer(s[api.PLAN_ROWS], api.ROW_DTYPE).reshape(N, N_OBS, M, 6)
        sfc = np.frombuffer(s[api.PLAN_SFC], api.BOX_DTYPE).reshape(N, M)
        x, obj = np.frombuffer(s[api.PLAN_PLAN], np.float64).reshape(N, NV), np.frombuffer(s[api.PLAN_OBJECTIVE], np.float64)
        info = np.frombuffer(s[api.PLAN_INFO], api.INFO_DTYPE)
        for q in range(N):
            ag = oracle.make_agent(p0=hdr["p0"][q], v0=hdr["v0"][q], a0=hdr["a0"][q], goal=hdr["goal"][q], next_waypoint=hdr["next_waypoint"][q],
                                   vmax=hdr["vmax"][q], amax=hdr["amax"][q], radius=hdr["radius"][q], nominal_velocity=hdr["nominal_velocity"][q],
                                   n_obs=N_OBS)
            lsc = np.zeros((N_OBS, M, 6), oracle.LSC_DTYPE)
            lsc["nrm"][..., 0], lsc["nrm"][..., 1], lsc["nrm"][..., 2], lsc["d"] = rows["nx"][q], rows["ny"][q], rows["nz"][q], rows["b"][q]
            box = np.zeros(M, oracle.BOX_DTYPE)
            box["bmin"], box["bmax"] = sfc["bmin"][q], sfc["bmax"][q]
            o = oracle.solve(cls, ag, lsc, box)
            assert o["status"] == 0, (k, q)
            assert abs(o["obj"] - obj[q]) <= 1e-8 * max(1.0, abs(o["obj"])), (k, q, o["obj"], obj[q])
            floor = bool(info["flags"][q] & (api.INFO_FLOOR_ACCEPTED | api.INFO_REMEMBERED))
            dxq = np.abs(o["x"] - x[q]).max()
            if dxq > 2e-6 and not floor:
                stat, eqv, iqv = H.kkt_from_primal(oracle, cls, ag, lsc, box, x[q])
                assert stat <= 1e-8 and eqv <= 1e-8 and iqv <= 1e-8, (k, q, dxq, stat, eqv, iqv)
                floor = True
            assert dxq <= (5e-5 if floor else 2e-6), (k, q, floor, dxq)


def test_the_obstacle_safety_figures_are_the_oracles(api, oracle, env, flown):
    """LSCQP_PLAN_OBS_SAFETY against oracle.safety_obstacles on the chain's own plans and table, at the bar tests/test_post.py holds the
    standalone kernel to: the ratio within 1e-5 (one float32 ulp of a 10 m coordinate in the Bernstein evaluation)."""
    W = env["W"]
    cls = oracle.make_class(M=M, dim=DIM, use_sfc=True, comm_range=0.0, world_min=W["world_min"], world_max=W["world_max"])
    same = 0
    for k, s in enumerate(flown["snaps"]):
        tab = _table(api, s)
        x = np.frombuffer(s[api.PLAN_PLAN], np.float64).reshape(N, NV)
        want = oracle.safety_obstacles(cls, N, x, RADIUS, DOWNWASH, np.c_[tab["position"], tab["radius"], tab["downwash"]], 2, 0.1)
        got = np.frombuffer(s[16 + api.PLAN_OBS_SAFETY], api.SAFETY_OBS_DTYPE)
        assert np.abs(got["safety_ratio_obs"] - want[:, 0]).max() <= 1e-5, k
        same += int((got["closest_obstacle"] == want[:, 1].astype(np.int32)).sum())
    assert same >= 0.98 * K * N, same


def test_the_graph_replays_the_eager_chain_with_three_more_nodes_than_the_twin(api, torch_cuda, env, flown):
    W = env["W"]
    plan = make_plan(api, env["sol"], env["wmap"])
    plan.set_obstacles(env["models"], obstacle_param(api))
    snaps = fly(api, torch_cuda, plan, W["starts"], W["goals"], K, graph=True)
    for k in range(K):
        assert snaps[k] == flown["snaps"][k], (k, [i for i in range(19) if snaps[k][i] != flown["snaps"][k][i]])
    assert plan.graph_nodes() == flown["twin_nodes"] + 3
    plan.close()
    # without the safety figures: two more
    a, b = make_plan(api, env["sol"], env["wmap"], safety=0), make_plan(api, env["sol"], env["wmap"], safety=0)
    a.set_obstacles(env["models"], obstacle_param(api))
    for p in (a, b):
        fly(api, torch_cuda, p, W["starts"], W["goals"], 2, graph=True, keep=lambda *_: None)
    assert a.graph_nodes() == b.graph_nodes() + 2 and b.graph_nodes() > 0
    assert a.get_obstacles(api.PLAN_OBS_CLOCK)[0] == 2
    a.close(), b.close()


def test_taking_the_obstacles_away_gives_the_twins_chain_back(api, torch_cuda, env, flown):
    """After set_obstacles(None) and a reset: the twin's node count and, over ten replans, the twin's buffers; no obstacle buffer is left."""
    W = env["W"]
    plan = make_plan(api, env["sol"], env["wmap"])
    plan.set_obstacles(env["models"], obstacle_param(api))
    fly(api, torch_cuda, plan, W["starts"], W["goals"], 3, graph=True, keep=lambda *_: None)
    plan.set_obstacles(None)
    assert plan.graph_nodes() == 0 and plan.obstacle_pointer(api.PLAN_OBS_TABLE) == (None, 0) and len(plan.get_obstacles()) == 0
    snaps = fly(api, torch_cuda, plan, W["starts"], W["goals"], 10, graph=True)
    assert plan.graph_nodes() == flown["twin_nodes"]
    for k in range(10):
        assert snaps[k] == flown["twin"][k], (k, [i for i in range(19) if snaps[k][i] != flown["twin"][k][i]])
    plan.close()


def test_a_second_reset_flies_the_same_thirty_replans(api, torch_cuda, env, flown):
    """... which shows that the reset zeroes the clock (and puts the table back)."""
    W = env["W"]
    again = fly(api, torch_cuda, flown["plan"], W["starts"], W["goals"], K, graph=True)
    assert all(again[k] == flown["snaps"][k] for k in range(K))


def test_refusals_of_the_setter_and_the_step_before_the_reset(api, torch_cuda, env):
    W, sol, wmap, m = env["W"], env["sol"], env["wmap"], env["models"]
    plan = make_plan(api, sol, wmap, n_obs=1)
    with pytest.raises(api.LscqpError, match="n_dyn exceeds the plan's row slots") as e:
        plan.set_obstacles(m)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    plan.set_obstacles(m[:1])  # (one obstacle and no agent slot: legal)
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_obstacles: lscqp_plan_reset must come before the next step"):
        plan.step()
    with pytest.raises(api.LscqpError, match="lscqp_plan_reset must come before"):
        plan.step(graph=True)
    plan.reset(W["starts"], W["goals"])
    plan.step()
    torch_cuda.cuda.synchronize()
    assert (plan.get(api.PLAN_IN_RANGE) == N - 1).all() and plan.get_obstacles(api.PLAN_OBS_CLOCK)[0] == 1
    bad = m[:1].copy()
    bad["speed"][0] = 0.0
    with pytest.raises(api.LscqpError, match="model 0: speed <= 0"):
        plan.set_obstacles(bad)
    plan.step()  # (a refused call leaves the plan as it was: no reset asked for)
    plan.close()
    bvc = api.Plan(sol, wmap, N, N_OBS, agents(api, N), constraint_mode=api.GEN_BVC, sfc_mode=api.SFC_FROM_POINT, optimize_goal=False, closed_loop=True,
                   prediction_mode=api.TRAJ_FROM_POSITION, initial_traj_mode=api.TRAJ_FROM_POSITION)
    with pytest.raises(api.LscqpError, match="constraint_mode must be LSCQP_GEN_LSC") as e:
        bvc.set_obstacles(m)
    assert e.value.code == api.ERR_UNSUPPORTED
    bvc.close()


def test_two_missions_in_one_partitioned_plan_each_fly_the_single_plan(api, torch_cuda, env, flown):
    """Two copies of the six agents as two missions of one plan, the obstacles shared like the map: each mission's slice of every
    per-agent buffer is the single plan's, bit for bit (ids in LSCQP_PLAN_BUF_SAFETY are global: the second copy's are shifted by six)."""
    W = env["W"]
    plan = api.Plan(env["sol"], env["wmap"], 2 * N, N_OBS, agents(api, 2 * N), constraint_mode=api.GEN_LSC, sfc_mode=api.SFC_FROM_POINT, optimize_goal=False,
                    closed_loop=True, safety_samples=2, record_time_step=0.1, mission_offsets=[0, N, 2 * N])
    plan.set_obstacles(env["models"], obstacle_param(api))
    snaps = fly(api, torch_cuda, plan, np.tile(W["starts"], (2, 1)), np.tile(W["goals"], (2, 1)), K, graph=True)
    plan.close()
    per_agent = [w for w in PLAN_BUFFERS if w != api.PLAN_SAFETY] + [16 + api.PLAN_OBS_SAFETY]
    for k in range(K):
        for w in per_agent:
            one = flown["snaps"][k][w]
            assert snaps[k][w] == one + one, (k, w)
        saf = np.frombuffer(snaps[k][api.PLAN_SAFETY], api.SAFETY_DTYPE).copy()
        saf["closest_agent"][N:] -= N
        one = flown["snaps"][k][api.PLAN_SAFETY]
        assert saf.tobytes() == one + one, k
        assert snaps[k][16 + api.PLAN_OBS_TABLE] == flown["snaps"][k][16 + api.PLAN_OBS_TABLE]


def test_two_owners_of_three_agents_each_equal_the_single_plan(api, torch_cuda, env, flown):
    """As tests/test_plan.py: test_plan_sharded_over_two_owners_equals_the_single_plan -- two plans own agents 0-2 and 3-5, each advances its
    own copy of the obstacle table, the owners' slices of plan, state and goal are exchanged through the host after every replan."""
    W, h = env["W"], N // 2
    parts = [make_plan(api, env["sol"], env["wmap"], n=h, n_total=N, first=f, safety=0) for f in (0, h)]
    for p in parts:
        p.set_obstacles(env["models"], obstacle_param(api))
        p.reset(W["starts"], W["goals"])
    for k in range(K):
        for p in parts:
            p.step(graph=True)
        torch_cuda.cuda.synchronize()
        s = flown["snaps"][k]
        for w, per in ((api.PLAN_PLAN, NV), (api.PLAN_STATE, 9), (api.PLAN_GOAL, 3)):
            full = [p.get(w).reshape(N, per) for p in parts]
            merged = np.concatenate([full[0][:h], full[1][h:]])
            assert merged.tobytes() == s[w], (k, w)
            for p in parts:
                p.put(w, merged)
        for w in (api.PLAN_ROWS, api.PLAN_STATUS, api.PLAN_IN_RANGE, api.PLAN_OBJECTIVE):
            assert raw(api, parts[0], w) + raw(api, parts[1], w) == s[w], (k, w)
        for p in parts:
            assert raw(api, p, api.PLAN_OBS_TABLE, obstacle=True) == s[16 + api.PLAN_OBS_TABLE], k
    for p in parts:
        p.close()


def test_a_plane_mission_with_one_straight_obstacle_eager_equals_graph(api, torch_cuda):
    """A 2-D class (M = 5, no corridors): four agents swap the corners of a square at z_2d, a straight obstacle crosses it in their plane."""
    z = 1.0
    starts = np.array([[-2.0, -2.0, z], [2.0, -2.0, z], [2.0, 2.0, z], [-2.0, 2.0, z]])
    goals = -starts
    goals[:, 2] = z
    sol = api.Solver(api.make_desc(M=M, dim=2, dt=DT, comm_range=0.0, use_sfc=False))
    models = api.obstacle_models([dict(type="straight", start=[-1.5, 0.2, z], goal=[1.5, -0.2, z], size=0.3, speed=0.3, max_acc=0.5, downwash=1.0)])
    out = []
    for graph in (False, True):
        plan = api.Plan(sol, None, 4, 4, agents(api, 4), constraint_mode=api.GEN_LSC, optimize_goal=False, closed_loop=True, safety_samples=2,
                        record_time_step=0.1, z_2d=z)
        plan.set_obstacles(models)
        out.append(fly(api, torch_cuda, plan, starts, goals, 10, graph=graph))
        assert (plan.get(api.PLAN_STATUS) == 0).all() and plan.get_obstacles(api.PLAN_OBS_CLOCK)[0] == 10
        assert (graph and plan.graph_nodes() > 0) or (not graph and plan.graph_nodes() == 0)
        plan.close()
    assert out[0] == out[1]
    rows = np.frombuffer(out[0][-1][api.PLAN_ROWS], api.ROW_DTYPE).reshape(4, 4, M, 6)
    assert (rows["nz"][:, 0] == 0).all() and np.abs(rows["nx"][:, 0]).max() > 0
    sol.close()


def test_a_shared_table_is_the_one_table_case_of_the_tables_per_mission(api, torch_cuda):
    """The plane mission above, three replans eager and by graph.  A plan with one shared table keeps it as one table of the per-mission
    layout and moves it by the per-mission entries: as many graph nodes as a plan of one mission that owns the same obstacle, one clock
    word, a table of n_dyn entries, every buffer of every replan that plan's, and safety figures that are lscqp_safety_obstacles_device's
    on the plans and the table the chain left."""
    torch, z = torch_cuda, 1.0
    starts = np.array([[-2.0, -2.0, z], [2.0, -2.0, z], [2.0, 2.0, z], [-2.0, 2.0, z]])
    goals = -starts
    goals[:, 2] = z
    sol = api.Solver(api.make_desc(M=M, dim=2, dt=DT, comm_range=0.0, use_sfc=False))
    models = api.obstacle_models([dict(type="straight", start=[-1.5, 0.2, z], goal=[1.5, -0.2, z], size=0.3, speed=0.3, max_acc=0.5, downwash=1.0)])
    ag = agents(api, 4)
    d_radius, d_downwash = torch.from_numpy(ag["radius"].copy()).cuda(), torch.from_numpy(ag["downwash"].copy()).cuda()
    flights, nodes = {}, {}
    for owned in (False, True):
        for graph in (False, True):
            plan = api.Plan(sol, None, 4, 4, ag, constraint_mode=api.GEN_LSC, optimize_goal=False, closed_loop=True, safety_samples=2, record_time_step=0.1,
                            z_2d=z)
            plan.set_mission_obstacles([models]) if owned else plan.set_obstacles(models)
            assert plan.obstacle_pointer(api.PLAN_OBS_CLOCK)[1] == 4 and plan.obstacle_pointer(api.PLAN_OBS_TABLE)[1] == len(models) * api.OBSTACLE_DTYPE.itemsize
            flights[owned, graph] = fly(api, torch, plan, starts, goals, 3, graph=graph)
            nodes[owned, graph] = plan.graph_nodes()
            assert plan.get_obstacles(api.PLAN_OBS_CLOCK).tolist() == [3]
            if not owned and not graph:
                for k, s in enumerate(flights[owned, graph]):
                    d_want = torch.zeros(4 * api.SAFETY_OBS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
                    up = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()  # noqa: E731
                    sol.safety_obstacles_device(4, 0, 4, 2, 0.1, up(s[api.PLAN_PLAN]), d_radius, d_downwash, len(models), up(s[16 + api.PLAN_OBS_TABLE]), d_want,
                                                z_2d=z)
                    torch.cuda.synchronize()
                    assert s[16 + api.PLAN_OBS_SAFETY] == d_want.cpu().numpy().tobytes(), k
                    assert np.isfinite(np.frombuffer(s[16 + api.PLAN_OBS_SAFETY], api.SAFETY_OBS_DTYPE)["safety_ratio_obs"]).all()
            plan.close()
    assert flights[False, False] == flights[False, True] == flights[True, False] == flights[True, True]
    assert nodes[False, True] == nodes[True, True] > 0 and nodes[False, False] == nodes[True, False] == 0
    sol.close()
