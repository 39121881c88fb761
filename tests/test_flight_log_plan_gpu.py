"""The flight log inside a plan's chain (include/lscqp.h, "the flight log": lscqp_plan_set_flight_log): the reference's own logged mission
flown eagerly and through the graph, free flights through lscqp_plan_run against a stepped twin, a mission with dynamic obstacles, and the
setter's lifecycle."""
import numpy as np
import pytest

from tests import flight_log_reference as FL
from tests import helpers as H
from tests import obstacle_reference as R
from tests import record_reference as RR
from tests import waypoint_cases as WC
from tests import waypoint_device as WD
from tests.test_record_plan_gpu import _replay, _scripted_mission, _scripted_plan

pytestmark = pytest.mark.gpu
DT, TIME_STEP, RTS = 0.2, 0.2, 0.1


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _half_unit(logged):
    """Half a unit of the sixth significant digit of a logged value (the precision of the reference's csv log; tests/helpers.py: log_units)."""
    logged = np.abs(np.asarray(logged, np.float64))
    with np.errstate(divide="ignore"):
        u = np.where(logged > 0, 10.0 ** (np.floor(np.log10(np.where(logged > 0, logged, 1.0))) - 5), 1e-6)
    return 0.5 * np.maximum(u, 1e-6)


def _bars(want):
    floor = np.repeat([1e-14, 1e-14 * 5 / DT, 1e-14 * 20 / DT ** 2], 3)  # (tests/test_flight_log_gpu.py: _bars)
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + floor


def test_the_references_logged_mission_eager_and_graph(api, torch_cuda):
    """79 scripted replans of the reference's forest10_10 mission, capacity 79, S = 2, eager and through the graph: equal bytes over the rows,
    and the graph has exactly one node more than the same plan with a record alone.

    Positions of row (r, s) against the log's pos[2r + s]: within tests/test_plan.py's standing bar for the replay, 440 units of the log's
    sixth digit.

    Sample 0 of every replan is the state the script fed (c0, c1, c2 are eliminated from it): the position is the fed one narrowed to
    float32, exactly; velocity and acceleration within (5/dt) 2 ulp32(|c|max) and (20/dt^2) 4 ulp32(|c|max) -- the float32 rounding of the
    three control points they are differences of -- plus the log's half unit of the sixth digit.  Derived, not measured.

    Sample 1 (t = 0.1, inside segment 0) depends on the QP's optimum against CPLEX's: tests/test_plan.py already holds the replay's
    positions, velocities and accelerations at that time to the log -- per (replan, agent) within the fixture's own match + 40 units, and
    440 units at most -- and those bars are used here, on the float32 values of the device log."""
    torch = torch_cuda
    W, m = _scripted_mission()
    K, N = m["K"], m["N"]
    logs, nodes = {}, {}
    for graph in (False, True):
        sol, wmap, plan = _scripted_plan(api, W, N, 0.1)
        plan.set_flight_log(K)
        figures, _ = _replay(api, torch, plan, W, m, graph)
        rec = plan.record()
        assert rec.log_rows()[0].tolist() == [K] and rec.log_rows()[1].tolist() == [0]
        logs[graph] = rec.log(0)
        for bit, field in enumerate(FL.FLAG_FIELDS):
            assert int(((logs[graph][1] >> bit) & 1).sum()) == int(figures[field][0]), field
        nodes[graph] = plan.graph_nodes()
        plan.close()
    sol, wmap, plain = _scripted_plan(api, W, N, 0.1)
    _replay(api, torch, plain, W, m, True)
    assert nodes[True] == plain.graph_nodes() + 1 and nodes[False] == 0
    plain.close()
    for a, b in zip(logs[False], logs[True]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    st, fl, ob = logs[True]
    assert st.shape == (K, N, 2, 9) and fl.shape == (K, N) and ob.shape == (K, 0, 4) and not (fl & (FL.FLAG_QP_FAILED | FL.FLAG_GOAL_FAILED | FL.FLAG_WAYPOINT)).any()
    S = H.load_golden("sim_log_states")
    lp, lv, la = (np.array(S[f]) for f in ("pos", "vel", "acc"))
    match = np.zeros((K, N))
    for r in H.load_golden("kat_log_pipeline")["replay"]:
        match[r["replan"], r["agent"]] = r["match"]
    worst = {0: 0.0, 1: 0.0}
    for r in range(K):
        for s in (0, 1):
            for a in range(N):
                for i in (0, 1):
                    worst[s] = max(worst[s], H.log_units(float(st[r, a, s, i]), lp[2 * r + s, a, i]))
    assert worst[0] <= 440 and worst[1] <= 440, worst
    # sample 0: the fed state
    fed = m["state"]  # (K, N, 9)
    assert np.array_equal(st[:, :, 0, 0:2], np.float32(fed[:, :, 0:2])) and (st[:, :, :, 2] == np.float32(W["z_2d"])).all()
    c0, c1 = fed[..., 0:2], fed[..., 0:2] + fed[..., 3:5] * DT / 5
    c2 = fed[..., 0:2] + 2 * fed[..., 3:5] * DT / 5 + fed[..., 6:8] * DT ** 2 / 20
    cmax = np.maximum(np.maximum(np.abs(c0), np.abs(c1)), np.abs(c2))
    bar_v = (5 / DT) * 2 * _ulp32(cmax) + _half_unit(fed[..., 3:5])
    bar_a = (20 / DT ** 2) * 4 * _ulp32(cmax) + _half_unit(fed[..., 6:8])
    dv, da = np.abs(st[:, :, 0, 3:5] - fed[..., 3:5]), np.abs(st[:, :, 0, 6:8] - fed[..., 6:8])
    print("sample 0: velocity off by at most %.3e (bar %.3e), acceleration %.3e (bar %.3e)" % (dv.max(), bar_v.min(), da.max(), bar_a.min()))
    assert (dv <= bar_v).all() and (da <= bar_a).all()
    assert not st[:, :, :, 5].any() and not st[:, :, :, 8].any()
    # sample 1: test_plan.py's bars for the replay at t = 0.1
    top = 0.0
    for r in range(K):
        for a in range(N):
            err = 0.0
            for got, logged in ((st[r, a, 1, 0:2], lp[2 * r + 1, a]), (st[r, a, 1, 3:5], lv[2 * r + 1, a]), (st[r, a, 1, 6:8], la[2 * r + 1, a])):
                err = max(err, max(H.log_units(float(got[i]), logged[i]) for i in range(2)))
            assert err <= match[r, a] + 40, (r, a, err, match[r, a])
            top = max(top, err)
    print("sample 1: at most %.1f units of the log's sixth digit from the log (bar 440); positions %.1f / %.1f" % (top, worst[0], worst[1]))
    assert top <= 440


def test_free_flight_does_not_depend_on_check_every_and_equals_a_stepped_twin(api, torch_cuda):
    """Three missions of 10, 6 and 12 agents over one map (tests/test_worlds_plan_gpu.py's), flown by lscqp_plan_run with check_every 1 and
    16: the logs are byte-identical over the rows and rows[k] == record.replans[k].  A twin plan without a log, stepped one replan at a
    time, tells what LSCQP_PLAN_BUF_PLAN held at every replan: each row's states lie within one float32 ulp of the restatement of that plan
    (tests/test_flight_log_gpu.py's bars), the flags are the restatement's of the twin's status buffers.  The threshold is the one
    mission 1 meets at replan 8 of the twin's flight, so at least one mission freezes inside the flight."""
    from tests.test_worlds_plan_gpu import SIZES, _plan, _setup

    torch = torch_cuda
    W, sol, maps, off, starts, goals = _setup(api)
    n, MAX = int(off[-1]), 20
    M, dim, z = 10, 2, W["z_2d"]
    twin = _plan(api, sol, maps[0], W, n, mission_offsets=off)
    twin.set_record(0.1)
    twin.reset(starts, goals)
    held = []
    for r in range(MAX):
        twin.step(graph=True)
        torch.cuda.synchronize()
        held.append((twin.get(api.PLAN_PLAN).reshape(n, -1).copy(), twin.get(api.PLAN_HEADER)["p0"].copy(),
                     [twin.get(b).copy() for b in (api.PLAN_STATUS, api.PLAN_VALID, api.PLAN_GOAL_STATUS, api.PLAN_SFC_STATUS, api.PLAN_WAYPOINT_UPDATED)]))
    twin.close()
    plane = np.array(goals, float).copy()
    plane[:, 2] = float(np.float32(z))
    thr = float(RR.vector3_distance(held[8][1][off[1]:off[2]], plane[off[1]:off[2]]).max()) + 1e-3
    plan = _plan(api, sol, maps[0], W, n, mission_offsets=off)
    plan.set_record(thr)
    plan.set_flight_log(MAX)
    out = {}
    for every in (1, 16):
        plan.reset(starts, goals)
        plan.run(MAX, check_every=every)
        rec = plan.record()
        rows, over = rec.log_rows()
        got, _ = rec.download()
        assert rows.tolist() == got["replans"].tolist() and not over.any()
        out[every] = (rows.tolist(), [rec.log(k) for k in range(len(SIZES))])
    assert out[1][0] == out[16][0] and out[1][0][1] <= 9 and max(out[1][0]) <= MAX
    print("rows per mission:", out[1][0], "threshold %.4f" % thr)
    for la, lb in zip(out[1][1], out[16][1]):
        for a, b in zip(la, lb):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()
    for k, (st, fl, ob) in enumerate(out[1][1]):
        lo, hi = int(off[k]), int(off[k + 1])
        assert st.shape == (out[1][0][k], SIZES[k], 2, 9)
        for r in range(st.shape[0]):
            x, _, ints = held[r]
            want = FL.states_f64(x[lo:hi], M, dim, DT, 2, RTS, z)
            assert (np.abs(st[r].astype(np.float64) - want) <= _bars(want)).all(), (k, r)
            assert np.array_equal(fl[r], FL.flags_word(ints[0][lo:hi], ints[1][lo:hi], ints[2][lo:hi], ints[3][lo:hi], ints[4][lo:hi])), (k, r)
        for bit, field in enumerate(FL.FLAG_FIELDS):
            assert int(((fl >> bit) & 1).sum()) == int(got[field][k]), (k, field)
    plan.close()


def test_obstacle_rows_are_the_table_at_every_replans_clock(api, torch_cuda):
    """tests/test_obstacles_plan_gpu.py's room and agents with one straight and one spin obstacle, ten replans through the graph.  Row r of
    the obstacle columns is the table of clock r under that module's bars for the table: the straight obstacle bit for bit, the spin within
    one float32 ulp of the coordinate; the radius is the model's.  lscqp_plan_set_obstacles BEFORE lscqp_plan_set_flight_log gives the same
    rows as AFTER it."""
    from tests import test_obstacles_plan_gpu as OP

    torch = torch_cuda
    W = OP.world()
    sol = OP.make_solver(api, W)
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    specs = [OP.obstacle_specs()[0],
             dict(type="spin", axis=[3.0, 3.0, 3.5, 0.0, 0.0, 1.0], start=[3.3, 3.0, 3.5], size=0.1, speed=0.2, max_acc=1.0, downwash=1.0)]
    models = api.obstacle_models(specs)
    objs = [R.from_model(mo) for mo in models]
    assert isinstance(objs[1], R.Spin)
    K, logs = 10, {}
    for order in ("log first", "obstacles first"):
        plan = OP.make_plan(api, sol, wmap)
        plan.set_record(0.1)
        if order == "log first":
            plan.set_flight_log(K)
            plan.set_obstacles(models, OP.obstacle_param(api))
        else:
            plan.set_obstacles(models, OP.obstacle_param(api))
            plan.set_flight_log(K)
        plan.reset(W["starts"], W["goals"])
        for _ in range(K):
            plan.step(graph=True)
        torch.cuda.synchronize()
        rec = plan.record()
        assert rec.log_rows()[0].tolist() == [K]
        logs[order] = rec.log(0)
        plan.close()
    for a, b in zip(logs["log first"], logs["obstacles first"]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    st, fl, ob = logs["log first"]
    assert ob.shape == (K, 2, 4) and st.shape == (K, OP.N, 2, 9)
    for r in range(K):
        t = R.clock_time(r, OP.DT)
        p0, _ = objs[0].at(t)
        p1, _ = objs[1].at(t)
        assert np.array_equal(ob[r, 0, 0:3], p0.astype(np.float32)), r
        assert (np.abs(ob[r, 1, 0:3].astype(np.float64) - p1) <= np.spacing(np.abs(p1))).all(), r
        assert ob[r, 0, 3] == np.float32(objs[0].radius) and ob[r, 1, 3] == np.float32(objs[1].radius)
    assert not np.array_equal(ob[0, :, 0:3], ob[K - 1, :, 0:3])  # (they moved)
    sol.close()


def test_lifecycle_of_the_setter(api, torch_cuda):
    """Without a record the setter is refused and names lscqp_plan_set_record.  A step before the reset is refused and names the setter.  A
    new partition after it: the reset makes a log for that partition.  Taking the record away takes the log away, and the graph has the bare
    plan's node count again; a record alone has one node more than that, a record with a log two."""
    torch = torch_cuda
    W = WC.forest10()
    starts, goals = np.array(W["starts"], float), np.array(W["goals"], float)
    n = len(starts)
    sol, wmap, plan = WD.forest10_plan(api, W)
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_record") as e:
        plan.set_flight_log(4)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    plan.reset(starts, goals)
    for _ in range(2):  # (the first replan after a reset is enqueued eagerly: the second one captures the graph)
        plan.step(graph=True)
    bare = plan.graph_nodes()
    plan.set_record(0.1)
    plan.reset(starts, goals)
    for _ in range(2):
        plan.step(graph=True)
    assert bare >= 9 and plan.graph_nodes() == bare + 1  # (a plan that never had a log: the chain of a record alone)
    with pytest.raises(api.LscqpError, match="no log"):
        plan.record().log_rows()
    with pytest.raises(api.LscqpError, match="max_replans"):
        plan.set_flight_log(-1)
    plan.step(graph=True)  # (the refused call changed nothing)
    plan.set_flight_log(4)
    for graph in (False, True):
        with pytest.raises(api.LscqpError, match="lscqp_plan_set_flight_log: lscqp_plan_reset must come before the next step"):
            plan.step(graph=graph)
    plan.reset(starts, goals)
    for _ in range(6):
        plan.step(graph=True)
    torch.cuda.synchronize()
    assert plan.graph_nodes() == bare + 2
    rows, over = plan.record().log_rows()
    assert rows.tolist() == [4] and over.tolist() == [1] and plan.record().log(0)[0].shape == (4, n, 2, 9)
    # a new partition: the record and its log are made again at the reset
    off = np.array([0, 4, n])
    plan.set_missions(off)
    assert plan.record() is None
    plan.reset(starts, goals)
    for _ in range(2):
        plan.step(graph=True)
    rec = plan.record()
    assert rec.log_rows()[0].tolist() == [2, 2] and rec.log(0)[0].shape == (2, 4, 2, 9) and rec.log(1)[0].shape == (2, n - 4, 2, 9)
    pts = rec.points()
    assert rec.log(1)[0][1, :, :, 0:3].tobytes() == pts[4:].tobytes()
    # the log alone taken away, then the record
    plan.set_flight_log(0)
    plan.step(graph=True)
    with pytest.raises(api.LscqpError, match="no log"):
        plan.record().log_rows()
    assert plan.record().download()[0]["replans"].tolist() == [3, 3]
    plan.set_flight_log(4)
    plan.set_record(None)
    assert plan.record() is None
    plan.set_missions(None)
    plan.reset(starts, goals)
    for _ in range(2):
        plan.step(graph=True)
    assert plan.graph_nodes() == bare
    with pytest.raises(api.LscqpError, match="lscqp_plan_set_record"):
        plan.set_flight_log(4)
    plan.close()
    sol.close()


def test_closed_loop_tool_writes_every_missions_result_log(tmp_path):
    """tools/closed_loop.py missions=2, until_finished=6, log_csv=DIR: one file per mission in the reference's format -- the header, then
    6 replans x 2 samples of 10 agents x 12 fields; row (r, s) stands at r * 0.2 + s * 0.1; sample 0 of replan 0 is the start position at rest."""
    import json
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import closed_loop

    world = os.path.join(root, "tests", "golden", "forest10_world.json")
    log = closed_loop.run(world, missions=2, until_finished=6, log_csv=str(tmp_path))
    assert json.loads(json.dumps(log))["log_csv"] == [str(tmp_path / "mission_0.csv"), str(tmp_path / "mission_1.csv")]
    assert [m["replans"] for m in log["per_mission"]] == [6, 6]
    for k in range(2):
        lines = (tmp_path / ("mission_%d.csv" % k)).read_text().splitlines()
        assert len(lines) == 1 + 6 * 2 and lines[0] == ",".join(["id,t,px,py,pz,vx,vy,vz,ax,ay,az,planning_time"] * 10)
        rows = [ln.split(",") for ln in lines[1:]]
        assert all(len(r) == 120 for r in rows) and [r[1] for r in rows[:4]] == ["0", "0.1", "0.2", "0.3"] and rows[5][109] == "0.5"
        assert [r[0::12] for r in rows[:1]] == [[str(q) for q in range(10)]]
        assert rows[0][5:11] == ["0"] * 6 and rows[0][4] == "0.6"
    with pytest.raises(ValueError, match="until_finished"):
        closed_loop.run(world, missions=2, log_csv=str(tmp_path))
