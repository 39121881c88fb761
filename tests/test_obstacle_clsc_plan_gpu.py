"""Dynamic obstacles in a CLSC plan's replan chain (include/lscqp.h, "dynamic obstacles in the chain"; csrc/lscplan.hip).

The scenario is tests/test_obstacles_plan_gpu.py's -- the 3-D room, six agents on a ring, a straight obstacle and a patrol, n_obs = 7 row
slots per agent (slots 0, 1 the obstacles) -- with constraint_mode = GEN_CLSC and ten replans, flown once with static goals
(optimize_goal = False) and once with the goal LP (optimize_goal = True: current goal point = start, the waypoints at the mission goals,
so that the LP walks each goal point towards its waypoint under the last-segment rows of every slot, the obstacles' among them).

With static goals this scenario leaves EVERY QP of every replan INFEASIBLE, with the obstacles and without them, and the oracle agrees on the
chain's own rows: the six goal segments (last point -> antipodal goal) cross at the middle of the ring, and generateCLSC's last-segment
rows ask for half the collision distance plus half of a separation that is not there -- CLSC is made for goal points the LP keeps near
the agent.  The agents then hover on their initial trajectories; what is held of that flight is the chain itself (rows, graph, twin).
The flight with the goal LP moves (1 QP of 60 not OPTIMAL), and the partition and the two owners fly that one.

One eager flight per setting is made once per module (`flown`), with every buffer of every replan kept; the tests read it and leave it
unchanged."""
import numpy as np
import pytest

from tests import test_obstacles_plan_gpu as P

pytestmark = pytest.mark.gpu

N, M, DIM, DT, N_DYN, N_OBS, NV = P.N, P.M, P.DIM, P.DT, P.N_DYN, P.N_OBS, P.NV
K = 10
RESOLVE_AT = (1, 5, 9)
GOAL_MODES = [False, True]


def make_plan(api, sol, wmap, og, n_obs=N_OBS, n=N, n_total=None, first=0, safety=2, mission_offsets=None, radii=None):
    ag = P.agents(api, n if n_total is None else n_total)
    if radii is not None:
        ag["radius"] = radii
    return api.Plan(sol, wmap, n, n_obs, ag, n_total=n_total, first_agent=first,
                    constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_POINT, optimize_goal=og, closed_loop=True, safety_samples=safety,
                    record_time_step=0.1, mission_offsets=mission_offsets)


def start(api, plan, starts, goals, og):
    """Static goals: the goal points are the mission's.  Goal LP: AgentManager's start (current goal point = start position), the local
    agents' waypoints at the mission goals."""
    if og:
        plan.reset(starts)
        plan.put(api.PLAN_WAYPOINT, np.float32(goals[plan.first_agent:plan.first_agent + plan.n_agents]).astype(np.float64))
    else:
        plan.reset(starts, goals)


def fly(api, torch, plan, starts, goals, og, k, graph, keep=P.snapshot):
    start(api, plan, starts, goals, og)
    out = []
    for _ in range(k):
        plan.step(graph=graph)
        torch.cuda.synchronize()
        out.append(keep(api, plan))
    return out


@pytest.fixture(scope="module")
def env(api, torch_cuda):
    W = P.world()
    sol = P.make_solver(api, W)
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    yield dict(W=W, sol=sol, wmap=wmap, models=api.obstacle_models(P.obstacle_specs()))
    sol.close()


@pytest.fixture(scope="module")
def flown(api, torch_cuda, env):
    """Per goal mode: the plan, per replan the plans and goal points BEFORE the step and every buffer after it; the twin without obstacles
    (n_obs = 7) flown eagerly and its graph's node count."""
    W, out = env["W"], {}
    for og in GOAL_MODES:
        plan = make_plan(api, env["sol"], env["wmap"], og)
        plan.set_obstacles(env["models"], P.obstacle_param(api))  # (fails without the feature: LSCQP_ERR_UNSUPPORTED on a CLSC plan)
        start(api, plan, W["starts"], W["goals"], og)
        before, before_goal, snaps = [], [], []
        for _ in range(K):
            before.append(P.raw(api, plan, api.PLAN_PLAN))
            before_goal.append(P.raw(api, plan, api.PLAN_GOAL))
            plan.step()
            torch_cuda.cuda.synchronize()
            snaps.append(P.snapshot(api, plan))
        twin = make_plan(api, env["sol"], env["wmap"], og)
        twin_snaps = fly(api, torch_cuda, twin, W["starts"], W["goals"], og, K, graph=False)
        twin.step(graph=True)
        twin_nodes = twin.graph_nodes()
        twin.close()
        out[og] = dict(plan=plan, snaps=snaps, before=before, before_goal=before_goal, twin=twin_snaps, twin_nodes=twin_nodes)
    yield out
    for og in GOAL_MODES:
        out[og]["plan"].close()


def test_set_obstacles_is_accepted_on_a_clsc_plan_and_still_refused_on_bvc(api, torch_cuda, env, flown):
    """The flight itself is the acceptance; the figures: QP statuses, the least slack of an obstacle-slot row and the least obstacle
    safety ratio (printed and recorded in NOTES.md, never asserted: a reciprocal half margin against an obstacle that does not do its
    half can let the agent closer than an LSC row would)."""
    for og in GOAL_MODES:
        f = flown[og]
        worst, slack, failed = np.inf, np.inf, 0
        for r, s in enumerate(f["snaps"]):
            st = np.frombuffer(s[api.PLAN_STATUS], np.int32)
            failed += int((st != 0).sum())
            worst = min(worst, float(np.frombuffer(s[16 + api.PLAN_OBS_SAFETY], api.SAFETY_OBS_DTYPE)["safety_ratio_obs"].min()))
            slack = min(slack, float(P.obstacle_slack(api, s[api.PLAN_ROWS], s[api.PLAN_PLAN], s[api.PLAN_STATUS]).min()))
            assert np.frombuffer(s[16 + api.PLAN_OBS_CLOCK], np.int32)[0] == r + 1
        print("CLSC plan with obstacles, optimize_goal=%s: %d of %d QPs not OPTIMAL, least obstacle-row slack %.3e m, least obstacle safety ratio %.6f"
              % (og, failed, K * N, slack, worst))
        assert f["plan"].n_dyn == N_DYN and np.isfinite(worst)
    bvc = api.Plan(env["sol"], env["wmap"], N, N_OBS, P.agents(api, N), constraint_mode=api.GEN_BVC, sfc_mode=api.SFC_FROM_POINT, optimize_goal=False,
                   closed_loop=True, prediction_mode=api.TRAJ_FROM_POSITION, initial_traj_mode=api.TRAJ_FROM_POSITION)
    with pytest.raises(api.LscqpError, match="constraint_mode must be LSCQP_GEN_LSC or LSCQP_GEN_CLSC") as e:
        bvc.set_obstacles(env["models"])
    assert e.value.code == api.ERR_UNSUPPORTED
    bvc.close()


@pytest.mark.parametrize("og", GOAL_MODES)
def test_the_obstacle_slots_are_the_standalone_entrys_rows(api, torch_cuda, env, flown, og):
    """Slots [0, n_dyn) of LSCQP_PLAN_BUF_ROWS equal, bit for bit, one lscqp_generate_obstacle_rows_device(LSCQP_GEN_CLSC) call without
    obstacle goals on what the chain itself held: the table downloaded, the goal points as they stood BEFORE the step (the rows precede
    the goal LP), the planning agents' initial trajectories rebuilt from the previous plans (the whole-segment shift; on the first replan
    the agents hover)."""
    torch, sol, f = torch_cuda, env["sol"], flown[og]
    dev = torch.device("cuda", 0)
    up = lambda b, dt=np.uint8: torch.from_numpy(np.frombuffer(b, dt).copy()).to(dev)  # noqa: E731
    par = P.obstacle_param(api)
    d_ids = torch.from_numpy(np.tile(np.arange(N_DYN, dtype=np.int32), N)).to(dev)
    d_radius = torch.full((N,), P.RADIUS, dtype=torch.float64, device=dev)
    for k, s in enumerate(f["snaps"]):
        if k == 0:
            p0 = np.float32(env["W"]["starts"]).astype(np.float64)
            d_own = torch.from_numpy(np.broadcast_to(p0[:, None, None, :], (N, M, 6, 3)).copy().reshape(-1)).to(dev)
        else:
            d_own = torch.zeros(N * M * 18, dtype=torch.float64, device=dev)
            sol.shift_traj_device(N, up(f["before"][k], np.float64), d_own)
        d_rows = torch.full((N * N_OBS * M * 6 * 4,), np.nan, dtype=torch.float64, device=dev)
        sol.generate_obstacle_rows_device(api.GEN_CLSC, par, N, N_DYN, 0, d_own, d_ids, up(s[16 + api.PLAN_OBS_TABLE]), None, d_radius,
                                          up(f["before_goal"][k], np.float64), None, d_rows, N_OBS, 0)
        torch.cuda.synchronize()
        want = d_rows.cpu().numpy().reshape(N, N_OBS, M * 6 * 4)
        got = np.frombuffer(s[api.PLAN_ROWS], np.float64).reshape(N, N_OBS, M * 6 * 4)
        assert np.isnan(want[:, N_DYN:]).all()
        assert want[:, :N_DYN].tobytes() == got[:, :N_DYN].tobytes(), k
        r = np.frombuffer(s[api.PLAN_ROWS], api.ROW_DTYPE).reshape(N, N_OBS, M, 6)[:, :N_DYN]
        assert (np.abs(r["nx"]) + np.abs(r["ny"]) + np.abs(r["nz"]) > 0).all(), k  # a normal on every segment, the last one too


@pytest.mark.parametrize("og", GOAL_MODES)
def test_on_the_first_replan_the_agent_slots_are_a_clsc_plan_of_five_slots_without_obstacles(api, torch_cuda, env, flown, og):
    W = env["W"]
    twin = make_plan(api, env["sol"], env["wmap"], og, n_obs=N_OBS - N_DYN)
    t = fly(api, torch_cuda, twin, W["starts"], W["goals"], og, 1, graph=False)[0]
    twin.close()
    s = flown[og]["snaps"][0]
    got = np.frombuffer(s[api.PLAN_ROWS], np.float64).reshape(N, N_OBS, -1)[:, N_DYN:]
    want = np.frombuffer(t[api.PLAN_ROWS], np.float64).reshape(N, N_OBS - N_DYN, -1)
    assert got.tobytes() == want.tobytes() and np.abs(want).max() > 0
    assert s[api.PLAN_IN_RANGE] == t[api.PLAN_IN_RANGE] and (np.frombuffer(s[api.PLAN_IN_RANGE], np.int32) == N - 1).all()


@pytest.mark.parametrize("og", GOAL_MODES)
def test_the_graph_replays_the_eager_chain_with_three_more_nodes_than_the_twin(api, torch_cuda, env, flown, og):
    W, f = env["W"], flown[og]
    plan = make_plan(api, env["sol"], env["wmap"], og)
    plan.set_obstacles(env["models"], P.obstacle_param(api))
    snaps = fly(api, torch_cuda, plan, W["starts"], W["goals"], og, K, graph=True)
    for k in range(K):
        assert snaps[k] == f["snaps"][k], (k, [i for i in range(19) if snaps[k][i] != f["snaps"][k][i]])
    assert plan.graph_nodes() == f["twin_nodes"] + 3
    # taking the obstacles away gives the twin's chain back: its node count and its buffers, no obstacle buffer left
    plan.set_obstacles(None)
    assert plan.graph_nodes() == 0 and plan.obstacle_pointer(api.PLAN_OBS_TABLE) == (None, 0)
    snaps = fly(api, torch_cuda, plan, W["starts"], W["goals"], og, K, graph=True)
    assert plan.graph_nodes() == f["twin_nodes"]
    for k in range(K):
        assert snaps[k] == f["twin"][k], (k, [i for i in range(19) if snaps[k][i] != f["twin"][k][i]])
    plan.close()


@pytest.mark.parametrize("og", GOAL_MODES)
def test_three_replans_are_resolved_by_the_oracle_from_the_chains_buffers(api, oracle, env, flown, og):
    """The QP as tests/test_obstacles_plan_gpu.py holds it (objective 1e-8 relative; x 2e-6 m, a flagged or flat-valley point 5e-5 m with
    its KKT residuals at 1e-8); the verdicts agree where the chain's QP is not OPTIMAL.  With the goal LP: LSCQP_PLAN_BUF_GOAL_STATUS is
    oracle.goal_opt's verdict on the chain's rows (every slot, the obstacles' too), last corridor box, waypoint and the goal point as it
    stood before the step, and the goal point is its result as point3d -- float32, at most one float32 ulp apart as tests/test_plan.py
    holds the chain's goal points: the LP's step differs in the last bits of its fp64 value between the two implementations and the
    result is rounded to float32 afterwards."""
    from tests import helpers as H

    W, f = env["W"], flown[og]
    cls = oracle.make_class(M=M, dim=DIM, use_sfc=True, comm_range=0.0, world_min=W["world_min"], world_max=W["world_max"])
    way = np.float32(W["goals"]).astype(np.float64)
    moved = off_by_an_ulp = compared = kept = 0
    for k in RESOLVE_AT:
        s = f["snaps"][k]
        hdr = np.frombuffer(s[api.PLAN_HEADER], api.HEADER_DTYPE)
        rows = np.frombuffer(s[api.PLAN_ROWS], api.ROW_DTYPE).reshape(N, N_OBS, M, 6)
        sfc = np.frombuffer(s[api.PLAN_SFC], api.BOX_DTYPE).reshape(N, M)
        x, obj = np.frombuffer(s[api.PLAN_PLAN], np.float64).reshape(N, NV), np.frombuffer(s[api.PLAN_OBJECTIVE], np.float64)
        status = np.frombuffer(s[api.PLAN_STATUS], np.int32)
        info = np.frombuffer(s[api.PLAN_INFO], api.INFO_DTYPE)
        g_before = np.frombuffer(f["before_goal"][k], np.float64).reshape(N, 3)
        g_after = np.frombuffer(s[api.PLAN_GOAL], np.float64).reshape(N, 3)
        g_status = np.frombuffer(s[api.PLAN_GOAL_STATUS], np.int32)
        for q in range(N):
            lsc = np.zeros((N_OBS, M, 6), oracle.LSC_DTYPE)
            lsc["nrm"][..., 0], lsc["nrm"][..., 1], lsc["nrm"][..., 2], lsc["d"] = rows["nx"][q], rows["ny"][q], rows["nz"][q], rows["b"][q]
            box = np.zeros(M, oracle.BOX_DTYPE)
            box["bmin"], box["bmax"] = sfc["bmin"][q], sfc["bmax"][q]
            if og:
                st, goal, _ = oracle.goal_opt(cls, g_before[q], way[q], lsc, box[M - 1])
                assert (g_status[q] == 0) == (st == 0), (k, q, g_status[q], st)
                want = np.float32(goal if st == 0 else g_before[q])
                assert np.array_equal(hdr["goal"][q], np.float32(hdr["goal"][q]).astype(np.float64))  # held as point3d
                assert (np.abs(np.float32(hdr["goal"][q]) - want) <= np.spacing(np.maximum(np.abs(want), np.float32(1.0)))).all(), (k, q, hdr["goal"][q], want)
                off_by_an_ulp += int((np.float32(hdr["goal"][q]) != want).sum())
                compared += 3
                assert np.array_equal(g_after[q], hdr["goal"][q]), (k, q)  # LSCQP_PLAN_BUF_GOAL is the header's goal, whatever the QP said
                kept += int(status[q] != 0)
                moved += int(not np.array_equal(g_after[q], g_before[q]))
            ag = oracle.make_agent(p0=hdr["p0"][q], v0=hdr["v0"][q], a0=hdr["a0"][q], goal=hdr["goal"][q], next_waypoint=hdr["next_waypoint"][q],
                                   vmax=hdr["vmax"][q], amax=hdr["amax"][q], radius=hdr["radius"][q], nominal_velocity=hdr["nominal_velocity"][q],
                                   n_obs=N_OBS)
            o = oracle.solve(cls, ag, lsc, box)
            assert (o["status"] == 0) == (status[q] == 0), (k, q, o["status"], status[q])
            if status[q] != 0:
                continue
            assert abs(o["obj"] - obj[q]) <= 1e-8 * max(1.0, abs(o["obj"])), (k, q, o["obj"], obj[q])
            floor = bool(info["flags"][q] & (api.INFO_FLOOR_ACCEPTED | api.INFO_REMEMBERED))
            dxq = np.abs(o["x"] - x[q]).max()
            if dxq > 2e-6 and not floor:
                stat, eqv, iqv = H.kkt_from_primal(oracle, cls, ag, lsc, box, x[q])
                assert stat <= 1e-8 and eqv <= 1e-8 and iqv <= 1e-8, (k, q, dxq, stat, eqv, iqv)
                floor = True
            assert dxq <= (5e-5 if floor else 2e-6), (k, q, floor, dxq)
    if og:
        # == but for goal coordinates one float32 ulp away; tests/test_plan.py allows 8 of 1 580 on the logged mission (0.5 %), the same share
        # of these 54 is none -- one is allowed, the least a count can allow
        print("goal LP in the CLSC chain with obstacles: %d of %d goal coordinates one float32 ulp from oracle.goal_opt's, the rest ==; %d agents "
              "with a failed QP" % (off_by_an_ulp, compared, kept))
        assert off_by_an_ulp <= 1, off_by_an_ulp
        assert moved > 0  # the LP did walk goal points


def test_two_missions_in_one_partitioned_plan_each_fly_the_single_plan(api, torch_cuda, env, flown):
    """Two copies of the six agents as two missions of one plan, the obstacles shared like the map: each mission's slice of every
    per-agent buffer is the single plan's, bit for bit (ids in LSCQP_PLAN_BUF_SAFETY are global: the second copy's are shifted by six)."""
    W, f = env["W"], flown[True]
    plan = make_plan(api, env["sol"], env["wmap"], True, n=2 * N, mission_offsets=[0, N, 2 * N])
    plan.set_obstacles(env["models"], P.obstacle_param(api))
    snaps = fly(api, torch_cuda, plan, np.tile(W["starts"], (2, 1)), np.tile(W["goals"], (2, 1)), True, K, graph=True)
    plan.close()
    per_agent = [w for w in P.PLAN_BUFFERS if w != api.PLAN_SAFETY] + [16 + api.PLAN_OBS_SAFETY]
    for k in range(K):
        for w in per_agent:
            one = f["snaps"][k][w]
            assert snaps[k][w] == one + one, (k, w)
        saf = np.frombuffer(snaps[k][api.PLAN_SAFETY], api.SAFETY_DTYPE).copy()
        saf["closest_agent"][N:] -= N
        one = f["snaps"][k][api.PLAN_SAFETY]
        assert saf.tobytes() == one + one, k
        assert snaps[k][16 + api.PLAN_OBS_TABLE] == f["snaps"][k][16 + api.PLAN_OBS_TABLE]


def test_two_owners_of_three_agents_each_equal_the_single_plan(api, torch_cuda, env, flown):
    """Two plans own agents 0-2 and 3-5 (first_agent 0 and 3, n_total 6); the owners' slices of plan, state and goal are exchanged through
    the host after every replan.  The obstacle rows read the radii and goal points of the LOCAL slice: every agent has a radius of its own
    (and, with the goal LP, a goal point of its own), so an offset slip in either shows in owner 1.  The single plan with those radii is
    flown here."""
    W, h = env["W"], N // 2
    radii = np.array([0.15, 0.13, 0.17, 0.14, 0.16, 0.12])
    single = make_plan(api, env["sol"], env["wmap"], True, radii=radii)
    single.set_obstacles(env["models"], P.obstacle_param(api))
    ref = fly(api, torch_cuda, single, W["starts"], W["goals"], True, K, graph=True)
    single.close()
    hdr = np.frombuffer(ref[0][api.PLAN_HEADER], api.HEADER_DTYPE)
    assert np.array_equal(hdr["radius"], radii) and any(ref[k][api.PLAN_ROWS] != flown[True]["snaps"][k][api.PLAN_ROWS] for k in range(K))
    parts = [make_plan(api, env["sol"], env["wmap"], True, n=h, n_total=N, first=first, safety=0, radii=radii) for first in (0, h)]
    for p in parts:
        p.set_obstacles(env["models"], P.obstacle_param(api))
        start(api, p, W["starts"], W["goals"], True)
    for k in range(K):
        for p in parts:
            p.step(graph=True)
        torch_cuda.cuda.synchronize()
        s = ref[k]
        for w, per in ((api.PLAN_PLAN, NV), (api.PLAN_STATE, 9), (api.PLAN_GOAL, 3)):
            full = [p.get(w).reshape(N, per) for p in parts]
            merged = np.concatenate([full[0][:h], full[1][h:]])
            assert merged.tobytes() == s[w], (k, w)
            for p in parts:
                p.put(w, merged)
        for w in (api.PLAN_ROWS, api.PLAN_STATUS, api.PLAN_IN_RANGE, api.PLAN_OBJECTIVE):
            assert P.raw(api, parts[0], w) + P.raw(api, parts[1], w) == s[w], (k, w)
        for p in parts:
            assert P.raw(api, p, api.PLAN_OBS_TABLE, obstacle=True) == s[16 + api.PLAN_OBS_TABLE], k
    for p in parts:
        p.close()


def test_a_plane_mission_at_z_06_with_one_straight_obstacle(api, torch_cuda, oracle):
    """A 2-D class (M = 5, no corridors, the goal LP on) in the plane z_2d = 0.6 of the reference's launch files: four agents swap the
    corners of a square centred at (3, 1), a straight obstacle crosses it in their plane.  The obstacle's goal point is the origin in the
    reference (include/obstacle.hpp never sets it) -- OFF the plane: on the last segment the LSC record's normal has a z component and
    its obstacle point a z below 0.6, and the row of the 2-D QP and goal LP is n_x (x - p_x) + n_y (y - p_y) >= d, nothing of z
    (src/traj_optimizer.cpp:414-421).  Held: eager == graph; n_z == 0 in the obstacle slot on every segment and a normal on every segment;
    at three replans the obstacle slot against the restatement's rows, b = d + n_x p_x + n_y p_y, on the chain's own buffers at TOL_N /
    TOL_B, with record normals that do leave the plane; and oracle.goal_opt at dim 2, fed the obstacle's UNPACKED records (p, nrm, d) and
    the agents' rows, gives the chain's verdicts and goal points (float32, one ulp)."""
    from tests import hull_reference as R
    from tests import lscgen_checks as T
    from tests import obstacle_rows_reference as RR

    z, n = 0.6, 4
    zf = float(np.float32(z))
    centre = np.array([3.0, 1.0, 0.0])
    starts = np.array([[-2.0, -2.0, z], [2.0, -2.0, z], [2.0, 2.0, z], [-2.0, 2.0, z]]) + centre
    goals = 2 * centre - starts
    sol = api.Solver(api.make_desc(M=M, dim=2, dt=DT, comm_range=0.0, use_sfc=False))
    models = api.obstacle_models([dict(type="straight", start=[1.5, 1.2, z], goal=[4.5, 0.8, z], size=0.3, speed=0.3, max_acc=0.5, downwash=1.0)])
    out, before, before_goal = [], [], []
    for graph in (False, True):
        plan = api.Plan(sol, None, n, 4, P.agents(api, n), constraint_mode=api.GEN_CLSC, optimize_goal=True, closed_loop=True, safety_samples=2,
                        record_time_step=0.1, z_2d=z)
        plan.set_obstacles(models)
        start(api, plan, starts, goals, True)
        snaps = []
        for _ in range(10):
            if not graph:
                before.append(P.raw(api, plan, api.PLAN_PLAN))
                before_goal.append(P.raw(api, plan, api.PLAN_GOAL))
            plan.step(graph=graph)
            torch_cuda.cuda.synchronize()
            snaps.append(P.snapshot(api, plan))
        out.append(snaps)
        assert plan.get_obstacles(api.PLAN_OBS_CLOCK)[0] == 10
        assert (graph and plan.graph_nodes() > 0) or (not graph and plan.graph_nodes() == 0)
        plan.close()
    assert out[0] == out[1]
    failed = 0
    for s in out[0]:
        rows = np.frombuffer(s[api.PLAN_ROWS], api.ROW_DTYPE).reshape(n, 4, M, 6)[:, 0]
        assert (rows["nz"] == 0).all()
        nn = np.abs(rows["nx"]) + np.abs(rows["ny"])
        assert (nn[:, :M - 1] > 0).all() and (nn[:, M - 1] > 0).all()
        failed += int((np.frombuffer(s[api.PLAN_STATUS], np.int32) != 0).sum())
    print("2-D CLSC plan at z_2d = 0.6 with one obstacle: %d of %d QPs not OPTIMAL" % (failed, n * len(out[0])))
    dev = torch_cuda.device("cuda", 0)
    cls = oracle.make_class(M=M, dim=2, use_sfc=False, comm_range=0.0)
    way = np.float32(goals).astype(np.float64)
    leaves, off_by_an_ulp = 0, 0
    for k in (0, 4, 9):
        s = out[0][k]
        if k == 0:
            own = np.broadcast_to(np.float32(starts).astype(np.float64)[:, None, None, :], (n, M, 6, 3)).copy()
        else:
            d_own = torch_cuda.zeros(n * M * 18, dtype=torch_cuda.float64, device=dev)
            sol.shift_traj_device(n, torch_cuda.from_numpy(np.frombuffer(before[k], np.float64).copy()).to(dev), d_own, z_2d=z)
            torch_cuda.cuda.synchronize()
            own = d_own.cpu().numpy().reshape(n, M, 6, 3)
        assert (own[..., 2] == zf).all()
        table = np.frombuffer(s[16 + api.PLAN_OBS_TABLE], api.OBSTACLE_DTYPE)
        g_before = np.frombuffer(before_goal[k], np.float64).reshape(n, 3)
        hdr = np.frombuffer(s[api.PLAN_HEADER], api.HEADER_DTYPE)
        g_status = np.frombuffer(s[api.PLAN_GOAL_STATUS], np.int32)
        r = np.frombuffer(s[api.PLAN_ROWS], api.ROW_DTYPE).reshape(n, 4, M, 6)
        got = np.stack([r["nx"], r["ny"], r["nz"], r["b"]], axis=-1)
        for a in range(n):
            want, (rp, rn, rd) = RR.clsc_obstacle_rows(oracle, R, M, 2, DT, own[a], g_before[a], P.RADIUS, table[0], 3.0, None, records=True)
            T._hold(got[a, 0], want, what="chain 2-D z=0.6, replan %d agent %d: obstacle slot vs d + nx px + ny py" % (k, a))
            leaves += int(abs(rn[M - 1, 2]) > 1e-3 and 0.0 < rp[M - 1, 0, 2] < zf)
            lsc = np.zeros((4, M, 6), oracle.LSC_DTYPE)
            lsc["nrm"][1:, ..., 0], lsc["nrm"][1:, ..., 1], lsc["d"][1:] = r["nx"][a, 1:], r["ny"][a, 1:], r["b"][a, 1:]
            lsc["p"][0], lsc["nrm"][0], lsc["d"][0] = rp, rn[:, None, :], rd
            st, goal, _ = oracle.goal_opt(cls, g_before[a], way[a], lsc, None)
            assert (g_status[a] == 0) == (st == 0), (k, a, g_status[a], st)
            w32 = np.float32(goal if st == 0 else g_before[a])[:2]
            assert (np.abs(np.float32(hdr["goal"][a][:2]) - w32) <= np.spacing(np.maximum(np.abs(w32), np.float32(1.0)))).all(), (k, a, hdr["goal"][a], w32)
            off_by_an_ulp += int((np.float32(hdr["goal"][a][:2]) != w32).sum())
    print("2-D CLSC plan at z_2d = 0.6: %d of 12 last-segment records leave the plane; %d of 24 goal coordinates one ulp from oracle.goal_opt's" % (leaves, off_by_an_ulp))
    assert leaves >= 2
    sol.close()
