"""The mission record as the last node of a plan's chain, and plans flown to the finish (include/lscqp.h, "the mission record"):
lscqp_plan_set_record / lscqp_plan_record / lscqp_plan_run against the reference's logged mission, against the numpy restatement fed from
the plan's own buffers (tests/record_reference.py), and across partitions."""
import json
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import record_reference as RR
from tests import waypoint_cases as WC
from tests import waypoint_device as WD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TIME_STEP = 0.2


def _scripted_mission():
    """The reference's logged forest10_10 mission as tests/test_plan.py's `_mission` replays it: per replan the logged states and the waypoints
    the replay fixture inferred."""
    g = H.load_golden("kat_log_pipeline")
    S = H.load_golden("sim_log_states")
    W = WC.forest10()
    K, N = 79, 10
    pos, vel, acc = np.array(S["pos"]), np.array(S["vel"]), np.array(S["acc"])
    way = np.zeros((K, N, 3))
    way[..., 2] = W["z_2d"]
    for r in g["replay"]:
        way[r["replan"], r["agent"], :2] = r["waypoint"]
    state = np.concatenate([pos[0:2 * K:2], vel[0:2 * K:2], acc[0:2 * K:2]], axis=2)
    state[..., 2] = W["z_2d"]
    return W, dict(K=K, N=N, pos=pos, way=way, state=state, summary=S["summary"])


def _scripted_plan(api, W, N, threshold):
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    plan = api.Plan(sol, wmap, N, 9, WD.agents(api, W["radius"], N), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True,
                    z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1)
    if threshold is not None:
        plan.set_record(threshold)
    return sol, wmap, plan


def _replay(api, torch, plan, W, m, graph, with_record=True):
    starts = np.array(W["starts"], dtype=np.float64)
    plan.reset(starts, np.array(W["goals"], dtype=np.float64) if with_record else None)
    if with_record:  # (waypoint_mode 0: the reset made the desired goals the CURRENT goal points; the replay starts them at the start points)
        plan.put(api.PLAN_GOAL, np.float32(starts).astype(np.float64))
    for k in range(m["K"]):
        plan.put(api.PLAN_STATE, m["state"][k])
        plan.put(api.PLAN_WAYPOINT, m["way"][k])
        plan.step(graph=graph)
    torch.cuda.synchronize()
    assert (plan.get(api.PLAN_STATUS) == 0).all()
    return plan.record().download() if with_record else None


def test_the_logged_mission_through_the_plan(api, torch_cuda):
    """79 scripted replans with a record set (safety_samples 2, record_time_step 0.1).  Threshold 0.1: not finished, replans 79.  Threshold
    0.13: replan 78 starts within it, so finished with replans 79 and flight_time 78 x 0.2.  Eager and graph flights give identical records,
    and the graph has exactly one node more than the same plan without a record.

    Distance: against the float32 polyline through the log's first 158 positions, 103.0571.  The bar is derived, not measured:
    tests/test_plan.py holds every coordinate of the replay to the log within 440 units of the log's sixth digit (1e-5 m for coordinates
    of 1 .. 10 m), i.e. a position within delta = 440e-5 x sqrt(2) m (+ 1e-6 for the float32 rounding of a sample point); each of the 157
    segments of each of the 10 agents then changes by at most 2 delta.  Measured deviation: see NOTES.md section 27.

    Safety: at least 1 - 5e-6 (the bar of test_plan.py) and not below the summary's 1.02089 by more than the 5e-5 of tests/test_post.py."""
    torch = torch_cuda
    W, m = _scripted_mission()
    out = {}
    for thr, graph in ((0.13, False), (0.13, True), (0.1, True)):
        sol, wmap, plan = _scripted_plan(api, W, m["N"], thr)
        out[thr, graph] = _replay(api, torch, plan, W, m, graph)
        if graph:
            out["nodes", thr] = plan.graph_nodes()
        plan.close()
    sol, wmap, bare = _scripted_plan(api, W, m["N"], None)
    assert bare.record() is None
    _replay(api, torch, bare, W, m, True, with_record=False)
    nodes = bare.graph_nodes()
    bare.close()
    assert out["nodes", 0.13] == out["nodes", 0.1] == nodes + 1 and nodes >= 9
    (rec_e, dist_e), (rec_g, dist_g), (rec_1, dist_1) = out[0.13, False], out[0.13, True], out[0.1, True]
    assert rec_e.tobytes() == rec_g.tobytes() and dist_e.tobytes() == dist_g.tobytes()
    a, b = rec_g[0], rec_1[0]
    assert (b["finished"], b["replans"], b["flight_time"]) == (0, 79, -1.0)
    assert (a["finished"], a["replans"]) == (1, 79) and abs(a["flight_time"] - 78 * TIME_STEP) <= 1e-12
    pos = np.float32(m["pos"][:158])
    want = float(sum(RR.vector3_norm(pos[1:, q] - pos[:-1, q]).sum() for q in range(m["N"])))
    assert abs(want - 103.0571) < 5e-5
    delta = 440e-5 * np.sqrt(2.0) + 1e-6
    print("record distance %.6f, log polyline %.6f, deviation %.3e (bar %.3f); safety ratio %.6f (summary %.5f)"
          % (a["distance"], want, abs(a["distance"] - want), 2 * delta * 157 * 10, a["safety_ratio_agent"], m["summary"]["safety_ratio_agent"]))
    assert a["distance"] == b["distance"] and abs(a["distance"] - want) <= 2 * delta * 157 * 10
    assert a["safety_ratio_agent"] >= 1.0 - 5e-6 and a["safety_ratio_agent"] >= m["summary"]["safety_ratio_agent"] - 5e-5
    for r in (a, b):
        assert r["qp_failed"] == 0 and r["first_qp_failed_replan"] == -1 and r["goal_failed"] == 0 and r["truncated"] == 0 and r["waypoint_updates"] == 0
        assert r["vel_excess_ratio"].max() <= 1e-5 and r["acc_excess_ratio"].max() <= 1e-5 and 0 <= r["safety_agent"] < 10 and 0 <= r["safety_other"] < 10


def _feed(api, plan, ref):
    """One replan of the restatement from the buffers the plan's last replan left."""
    hdr = plan.get(api.PLAN_HEADER)
    ref.step(plan.record().points(), hdr["p0"], plan.get(api.PLAN_STATUS), plan.get(api.PLAN_GOAL_STATUS), plan.get(api.PLAN_SFC_STATUS),
             plan.get(api.PLAN_VALID), plan.get(api.PLAN_IN_RANGE), hdr["n_obs"], plan.get(api.PLAN_SAFETY), plan.get(api.PLAN_WAYPOINT_UPDATED))
    return hdr["p0"].copy()


def test_free_flight_equals_the_restatement_and_runs_to_the_finish(api, torch_cuda):
    """forest10 with the device's own waypoints, closed loop, one replan at a time: after every one of 22 replans the record equals the
    restatement fed from the downloaded buffers, exactly.  The largest goal distance at the start of replan 20 plus a millimetre is a threshold
    that finishes the mission by replan 20; lscqp_plan_run with check_every 1 and 7 (max_replans 40) then returns the same records bit for
    bit -- the restatement's over the stored points -- with finished = 1, and has enqueued whole batches up to the finishing replan.

    The issue expected "at least 21 replans enqueued", i.e. the threshold first met AT replan 20.  This flight does not approach its goals
    monotonically (one PIBT step can send an agent backwards): measured on MI355X, the largest goal distance is 7.1950 m at replan 16,
    7.2797 m at replan 19 and 7.2700 m at replan 20, so a threshold taken at replan 20 is first met at replan 16.  The test therefore takes
    the first replan that meets the threshold from the restatement and asserts the exact count: first + 1 replans with check_every 1, the next
    multiple of 7 with check_every 7."""
    torch = torch_cuda
    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    n = len(starts)
    sol, wmap, plan = WD.forest10_plan(api, W)
    plan.set_record(0.1)
    with pytest.raises(api.LscqpError, match="lscqp_plan_reset"):  # the record has no goals yet
        plan.step()
    plan.reset(starts, goals)
    ref = RR.Record(n, _plane(goals, W), 0.1, TIME_STEP)
    seen, p0s = [], []
    for r in range(22):
        plan.step(graph=True)
        torch.cuda.synchronize()
        p0s.append(_feed(api, plan, ref))
        seen.append((plan.record().points(), plan.get(api.PLAN_HEADER), [plan.get(b) for b in (api.PLAN_STATUS, api.PLAN_GOAL_STATUS, api.PLAN_SFC_STATUS,
                                                                                               api.PLAN_VALID, api.PLAN_IN_RANGE)],
                     plan.get(api.PLAN_SAFETY), plan.get(api.PLAN_WAYPOINT_UPDATED)))
        got, dist = plan.record().download()
        bad = RR.same_records(got, ref.records())
        assert not bad and np.array_equal(dist, ref.dist), (r, bad[:4])
    assert got["finished"][0] == 0 and got["replans"][0] == 22 and got["waypoint_updates"][0] > 0 and got["distance"][0] > 1.0
    far = [float(RR.vector3_distance(p, _plane(goals, W)).max()) for p in p0s]
    thr = far[20] + 1e-3
    first = min(r for r in range(21) if far[r] <= thr)  # (PIBT sends agents backwards at times: the distance need not fall from replan to replan)
    print("largest goal distance per replan:", " ".join("%.4f" % f for f in far), "-> threshold %.4f first met at replan %d" % (thr, first))
    want = RR.Record(n, _plane(goals, W), thr, TIME_STEP)
    for pts, hdr, ints, saf, wp in seen:
        want.step(pts, hdr["p0"], ints[0], ints[1], ints[2], ints[3], ints[4], hdr["n_obs"], saf, wp)
    assert first <= 20 and want.records()[0]["finished"] == 1 and want.records()[0]["replans"] == first + 1
    runs = {}
    for every in (1, 7):
        plan.set_record(thr)
        plan.reset(starts, goals)
        enqueued = plan.run(40, check_every=every)
        got, dist = plan.record().download()
        assert not RR.same_records(got, want.records()) and np.array_equal(dist, want.dist), every
        assert got["finished"][0] == 1 and got["replans"][0] == first + 1 and plan.record().unfinished() == 0
        assert enqueued == -(-(first + 1) // every) * every, (every, enqueued)  # whole batches, and not one more than needed
        runs[every] = (got.tobytes(), dist.tobytes())
    assert runs[1] == runs[7]
    plan.close()


def _plane(goals, W):
    g = np.array(goals, float).copy()
    g[:, 2] = float(np.float32(W["z_2d"]))  # (a 2-D mission: the desired goals are pinned to its plane, like the states)
    return g


def test_three_missions_one_of_them_already_there(api, torch_cuda):
    """forest10 twice plus a mission of three agents whose starts are their goals, in one plan: the trivial mission finishes at replan 0
    (flight_time 0, replans 1) and stays frozen; the two copies have identical records (ids relative to the mission), equal to the record of a
    ten-agent plan without a partition."""
    torch = torch_cuda
    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    n, steps = len(starts), 12
    sol, wmap, single = WD.forest10_plan(api, W)
    single.set_record(0.1)
    single.reset(starts, goals)
    off = np.array([0, n, n + 3, 2 * n + 3])
    many = api.Plan(sol, wmap, int(off[-1]), n - 1, WD.agents(api, W["radius"], int(off[-1])), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL,
                    optimize_goal=True, closed_loop=True, z_2d=W["z_2d"], safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT)
    many.set_record(0.1)  # before the partition: rebuilt for it at the reset
    many.set_missions(off)
    assert many.record() is None  # (the record of the old partition is gone)
    many.reset(np.concatenate([starts, starts[:3], starts]), np.concatenate([goals, starts[:3], goals]))
    assert many.record().unfinished() == 3
    assert single.run(steps, check_every=steps) == steps and many.run(steps, check_every=5) == steps
    one, dist_one = single.record().download()
    got, dist = many.record().download()
    assert (got["finished"][1], got["replans"][1], got["flight_time"][1], got["distance"][1]) == (1, 1, 0.0, 0.0) and many.record().unfinished() == 2

    def local(rec, k, base):
        r = rec[k:k + 1].copy()
        for f in ("safety_agent", "safety_other"):
            r[f] = np.where(r[f] >= 0, r[f] - base, r[f])
        return r.tobytes()

    assert local(got, 0, 0) == local(got, 2, n + 3) == local(one, 0, 0)
    assert np.array_equal(dist[:n], dist_one) and np.array_equal(dist[n + 3:], dist_one) and got["replans"][0] == steps and got["distance"][0] > 1.0
    many.close()
    single.close()


def test_plans_without_a_record_and_refused_calls(api, torch_cuda):
    """Without a record: lscqp_plan_record is NULL, lscqp_plan_run is refused, and a step gives the bits of a plan that never saw the call; taking
    a record away again gives the chain back node for node.  lscqp_plan_run needs closed_loop and the device's own waypoints; the record needs
    the safety figures; a reset with a record needs the goals."""
    torch = torch_cuda
    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    sol, wmap, plain = WD.forest10_plan(api, W)
    sol2, wmap2, other = WD.forest10_plan(api, W)
    assert other.record() is None
    with pytest.raises(api.LscqpError, match="no record") as e:
        other.run(5)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    other.set_record(0.1)
    assert other.record() is not None
    with pytest.raises(api.LscqpError, match="goal points") as e:
        other.reset(starts)
    other.set_record(None)
    assert other.record() is None
    for p in (plain, other):
        p.reset(starts, goals)
        for _ in range(3):
            p.step(graph=True)
    torch.cuda.synchronize()
    for b in (api.PLAN_PLAN, api.PLAN_STATE, api.PLAN_GOAL, api.PLAN_WAYPOINT):
        assert np.array_equal(plain.get(b), other.get(b)), b
    assert plain.graph_nodes() == other.graph_nodes() > 0
    other.set_record(0.1)
    other.reset(starts, goals)
    for bad in ((0, 1), (5, 0)):
        with pytest.raises(api.LscqpError, match="max_replans"):
            other.run(*bad)
    for p in (plain, other):
        p.close()
    n = len(starts)
    for kw, word in ((dict(closed_loop=False, waypoint_mode=api.WAYPOINT_GRID_PIBT), "closed_loop"), (dict(closed_loop=True, waypoint_mode=api.WAYPOINT_FROM_CALLER), "closed_loop")):
        p = api.Plan(sol, wmap, n, n - 1, WD.agents(api, W["radius"], n), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, z_2d=W["z_2d"],
                     safety_samples=2, record_time_step=0.1, **kw)
        p.set_record(0.1)
        p.reset(starts, goals)
        with pytest.raises(api.LscqpError, match=word) as e:
            p.run(5)
        assert e.value.code == api.ERR_INVALID_ARGUMENT
        p.close()
    p = api.Plan(sol, wmap, n, n - 1, WD.agents(api, W["radius"], n), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, z_2d=W["z_2d"])
    with pytest.raises(api.LscqpError, match="safety_samples") as e:
        p.set_record(0.1)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and p.record() is None
    p.close()
    p = api.Plan(sol, wmap, n, n - 1, WD.agents(api, W["radius"], n), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, z_2d=W["z_2d"],
                 safety_samples=2, record_time_step=0.1)
    p.set_record(0.1)
    with pytest.raises(api.LscqpError, match="desired goals"):  # (waypoint_mode 0 takes a reset without goals; with a record it does not)
        p.reset(starts)
    p.close()


def test_closed_loop_tool_flies_missions_until_finished():
    """tools/closed_loop.py missions=K, until_finished=MAX: one record per mission straight from the device, the summary stays JSON, and the
    figures of mission 0 -- the world's own -- hold the bars of test_closed_loop.py over however many replans were flown."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import closed_loop

    log = closed_loop.run(os.path.join(ROOT, "tests", "golden", "forest10_world.json"), missions=2, until_finished=32)
    back = json.loads(json.dumps(log))
    assert back["missions"] == 2 and back["agents"] == 20 and [m["mission"] for m in back["per_mission"]] == [0, 1]
    assert back["replans_enqueued"] == 32 and back["finished"] == sum(m["finished"] for m in back["per_mission"])  # (forest10 needs 79 replans)
    m0 = log["per_mission"][0]
    assert m0["finished"] == 0 and m0["replans"] == 32 and m0["flight_time_s"] == -1.0 and m0["flight_distance_m"] > 10.0
    assert m0["qp_failed"] == 0 and m0["first_qp_failed_replan"] == -1 and m0["truncated_agent_steps"] == 0 and m0["walk_bound_reached"] == 0
    assert m0["min_safety_ratio"] >= 1.0 - 5e-6 and m0["max_vel_excess"] <= 1e-5 and m0["max_acc_excess"] <= 1e-5 and m0["waypoints_updated"] > 20
    with pytest.raises(ValueError):
        closed_loop.run(os.path.join(ROOT, "tests", "golden", "forest10_world.json"), until_finished=5)
