"""The mission record on the device (include/lscqp.h, "the mission record"; csrc/lscrecord.hip): the stand-alone entry points on constructed
inputs -- no QP is solved -- against the numpy restatement (tests/record_reference.py).  The restatement is handed the sample points the
device wrote, so every field of every record and every agent's distance is compared exactly; the points themselves are held to one
float32 ulp of a float64 evaluation of the same plans."""
import numpy as np
import pytest

from tests import record_reference as RR

pytestmark = pytest.mark.gpu

M, DIM, DT, S, RECORD_DT, TIME_STEP, Z2D = 5, 2, 0.2, 2, 0.1, 0.2, 0.6
NV = DIM * M * 6
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)  # both sides of the wavefront (64) and of the workgroup's stride (256)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _inputs(api, rng, n, goals, near=None, wild=False):
    """One replan's inputs for n agents: random plans and figures; `near`: boolean (n,), the agents that start AT their goals."""
    scale = 1e3 if wild else 1.0
    x = rng.uniform(-4, 4, (n, NV)) * scale
    hdr = np.zeros(n, api.HEADER_DTYPE)
    hdr["p0"] = goals + rng.uniform(1.0, 2.0, (n, 3))
    if near is not None:
        hdr["p0"][near] = goals[near]
    hdr["n_obs"] = rng.integers(0, 6, n)
    saf = np.zeros(n, api.SAFETY_DTYPE)
    saf["safety_ratio"] = rng.uniform(1.0, 3.0, n) * (1e-3 if wild else 1.0)
    saf["closest_agent"] = rng.integers(0, n, n)
    saf["vel_excess_ratio"] = rng.uniform(-0.5, 0.5, (n, 3)) * scale
    saf["acc_excess_ratio"] = rng.uniform(-0.5, 0.5, (n, 3)) * scale
    ints = dict(status=rng.integers(0, 5, n), goal_status=rng.integers(0, 3, n), sfc_status=rng.integers(0, 2, n), valid=rng.integers(0, 2, n),
                in_range=rng.integers(0, 9, n) * (100 if wild else 1), wp=rng.integers(0, 2, n))
    return dict(x=x, hdr=hdr, saf=saf, **{k: v.astype(np.int32) for k, v in ints.items()})


def _step(torch, rec, ref, I, with_wp=True):
    """The same replan on the device and, from the device's points, in the restatement.  Returns the points."""
    d = {k: _dev(torch, v) for k, v in I.items()}
    rec.step_device(d["hdr"], d["x"], d["status"], d["goal_status"], d["sfc_status"], d["valid"], d["in_range"], d["saf"], d["wp"] if with_wp else None)
    pts = rec.points()
    ref.step(pts, I["hdr"]["p0"], I["status"], I["goal_status"], I["sfc_status"], I["valid"], I["in_range"], I["hdr"]["n_obs"], I["saf"],
             I["wp"] if with_wp else None)
    return pts


def _check(rec, ref):
    got, dist = rec.download()
    bad = RR.same_records(got, ref.records())
    assert not bad, bad[:5]
    assert np.array_equal(dist, ref.dist)
    assert rec.unfinished() == ref.unfinished
    return got


def _solver(api):
    return api.Solver(api.make_desc(M=M, dim=DIM, dt=DT))


@pytest.mark.parametrize("partition", ["missions", "one"])
def test_records_equal_the_restatement_at_every_size(api, torch_cuda, partition):
    """Missions of 1, 2, 63, 64, 65, 255, 256, 257 and 513 agents in one call, and the same agents as ONE mission (offsets = NULL): four
    replans of random figures over every status value, the missions finishing at different replans.  Exact equality; the device's points
    within one float32 ulp of the float64 evaluation (the device forms the same sum in float64 in another order and rounds it to float32:
    the result is one of the two float32 neighbours of the exact value; derived, not measured)."""
    torch = torch_cuda
    off = np.concatenate([[0], np.cumsum(SIZES)])
    n = int(off[-1])
    offsets = off if partition == "missions" else None
    rng = np.random.default_rng(5)
    goals = rng.uniform(-4, 4, (n, 3))
    sol = _solver(api)
    rec = api.Record(sol, n, offsets, S, RECORD_DT, TIME_STEP, Z2D, goal_threshold=0.5)
    rec.reset(goals)
    ref = RR.Record(n, goals, 0.5, TIME_STEP, offsets)
    finished_at = {0: 1, 3: 0, 5: 2, 8: 3}  # mission -> the replan it starts within the threshold
    for r in range(4):
        near = np.zeros(n, bool)
        for k, at in finished_at.items():
            if at == r and partition == "missions":
                near[off[k]:off[k + 1]] = True
        if partition == "one" and r == 2:
            near[:] = True
        I = _inputs(api, rng, n, goals, near)
        pts = _step(torch, rec, ref, I)
        got = _check(rec, ref)
        if r == 0:
            want = RR.points_f64(I["x"], M, DIM, DT, S, RECORD_DT, Z2D)
            # (+ 1e-14: what two float64 evaluations of a sum of six terms of size 4 can differ by, for a value that happens to lie near 0)
            assert (np.abs(pts.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-14).all()
            assert (pts[..., 2] == np.float32(Z2D)).all()
    if partition == "missions":
        assert got["finished"].tolist() == [1, 0, 0, 1, 0, 1, 0, 0, 1] and got["replans"].tolist() == [2, 4, 4, 1, 4, 3, 4, 4, 4]
        assert got["flight_time"][[0, 3, 5, 8]].tolist() == [1 * TIME_STEP, 0.0, 2 * TIME_STEP, 3 * TIME_STEP] and got["flight_time"][1] == -1.0
        assert rec.unfinished() == 5
    else:
        assert got["finished"].tolist() == [1] and got["replans"].tolist() == [3] and rec.unfinished() == 0
    assert got["qp_failed"].sum() > 0 and got["truncated"].sum() > 0 and got["first_qp_failed_replan"].max() >= 0
    rec.close()
    sol.close()


@pytest.mark.parametrize("where", ["first", "last", 63, 64, 256])
def test_an_agent_exactly_at_the_threshold_finishes_and_one_ulp_further_does_not(api, torch_cuda, where):
    """Goal (0, 0), position (0.375, 0.5), threshold 0.625: the float32 distance is exactly 0.625 and equality counts as finished.  One
    float32 ulp further out in y it does not.  The deciding agent is the first of its mission, the last, and at local indices 63, 64 and
    256 (the last lane of a wavefront, the first of the next, the first agent a lane meets on its second round); everybody else is AT its goal."""
    torch = torch_cuda
    size = 300
    off = np.array([0, 7, 7 + size, 7 + size + 5])
    n = int(off[-1])
    local = {"first": 0, "last": size - 1}.get(where, where)
    a = int(off[1]) + local
    rng = np.random.default_rng(11)
    goals = np.zeros((n, 3))
    goals[:, 2] = Z2D
    sol = _solver(api)
    for y, finishes in ((0.5, True), (float(np.nextafter(np.float32(0.5), np.float32(1.0))), False)):
        rec = api.Record(sol, n, off, S, RECORD_DT, TIME_STEP, Z2D, goal_threshold=0.625)
        rec.reset(goals)
        ref = RR.Record(n, goals, 0.625, TIME_STEP, off)
        I = _inputs(api, rng, n, goals, np.ones(n, bool))
        I["hdr"]["p0"][a] = [0.375, y, Z2D]
        _step(torch, rec, ref, I)
        got = _check(rec, ref)
        assert got["finished"].tolist() == [1, int(finishes), 1], (where, y)
        assert rec.unfinished() == (0 if finishes else 1)
        rec.close()
    sol.close()


def test_a_finished_mission_is_frozen_and_its_neighbours_are_not(api, torch_cuda):
    """Three missions; the middle one finishes at replan 1.  Further steps with wild inputs (plans a thousand times larger, every figure out of
    range) leave every byte of its record and its agents' distances alone and do change both neighbours'; the unfinished word counts 3, 2,
    ... down to 0 and stays there."""
    torch = torch_cuda
    off = np.array([0, 70, 140, 400])
    n = int(off[-1])
    rng = np.random.default_rng(3)
    goals = rng.uniform(-4, 4, (n, 3))
    sol = _solver(api)
    rec = api.Record(sol, n, off, S, RECORD_DT, TIME_STEP, Z2D, goal_threshold=0.25)
    rec.reset(goals)
    ref = RR.Record(n, goals, 0.25, TIME_STEP, off)
    mid = np.zeros(n, bool)
    mid[70:140] = True
    assert rec.unfinished() == 3
    _step(torch, rec, ref, _inputs(api, rng, n, goals))
    _step(torch, rec, ref, _inputs(api, rng, n, goals, mid))
    frozen, fdist = rec.download()
    assert frozen["finished"].tolist() == [0, 1, 0] and rec.unfinished() == 2
    for _ in range(2):
        _step(torch, rec, ref, _inputs(api, rng, n, goals, wild=True))
        got, dist = _check(rec, ref), rec.download()[1]
        assert got[1].tobytes() == frozen[1].tobytes() and np.array_equal(dist[70:140], fdist[70:140])
        assert got[0].tobytes() != frozen[0].tobytes() and got[2].tobytes() != frozen[2].tobytes()
        assert (dist[:70] > fdist[:70]).all() and (dist[140:] > fdist[140:]).all()
    assert got["safety_replan"].tolist()[0] >= 2 and got["max_in_range"][0] >= 100
    everyone = np.ones(n, bool)
    _step(torch, rec, ref, _inputs(api, rng, n, goals, everyone))
    assert rec.unfinished() == 0
    done = _check(rec, ref)
    _step(torch, rec, ref, _inputs(api, rng, n, goals, everyone, wild=True))
    assert rec.unfinished() == 0 and rec.download()[0].tobytes() == done.tobytes()
    rec.close()
    sol.close()


def test_ties_signed_excess_counts_and_no_waypoint_buffer(api, torch_cuda):
    """Two agents, two replans, all four safety ratios equal: the first replan and the lower id keep the minimum (with ITS closest agent).  A
    smaller ratio later does take over.  Excess values at or below zero leave the maxima at 0.  The counts over every status value, by hand.
    d_waypoint_updated = NULL leaves waypoint_updates at 0."""
    torch = torch_cuda
    n = 2
    goals = np.zeros((n, 3))
    sol = _solver(api)
    rec = api.Record(sol, n, None, S, RECORD_DT, TIME_STEP, Z2D, goal_threshold=0.1)
    rec.reset(goals)
    ref = RR.Record(n, goals, 0.1, TIME_STEP)
    rng = np.random.default_rng(2)
    for r in range(2):
        I = _inputs(api, rng, n, goals)
        I["saf"]["safety_ratio"] = 1.25
        I["saf"]["closest_agent"] = [1, 0] if r == 0 else [7, 7]
        I["saf"]["vel_excess_ratio"], I["saf"]["acc_excess_ratio"] = [[-0.5, 0.0, -1e-300]] * 2, [[-3.0, -0.0, 0.0]] * 2
        I["status"][:], I["goal_status"][:], I["sfc_status"][:], I["valid"][:] = [r, 4 - r], [0, 2], [1, 0], [1 - r, 1]
        I["in_range"][:], I["hdr"]["n_obs"] = [3, 4 + r], [3, 4]
        _step(torch, rec, ref, I, with_wp=False)
        got = _check(rec, ref)
    m = got[0]
    assert (m["safety_ratio_agent"], m["safety_replan"], m["safety_agent"], m["safety_other"]) == (1.25, 0, 0, 1)
    assert m["vel_excess_ratio"].tolist() == [0, 0, 0] and m["acc_excess_ratio"].tolist() == [0, 0, 0]
    assert (m["qp_failed"], m["first_qp_failed_replan"], m["goal_failed"], m["sfc_kept"], m["invalid"]) == (3, 0, 2, 2, 1)
    assert (m["max_in_range"], m["truncated"], m["waypoint_updates"], m["replans"], m["finished"]) == (5, 1, 0, 2, 0)
    I = _inputs(api, rng, n, goals)
    I["saf"]["safety_ratio"], I["saf"]["closest_agent"] = [1.25, 1.0], [1, 0]
    I["saf"]["vel_excess_ratio"][1] = [0.25, -1.0, 0.5]
    _step(torch, rec, ref, I)
    m = _check(rec, ref)[0]
    assert (m["safety_ratio_agent"], m["safety_replan"], m["safety_agent"], m["safety_other"]) == (1.0, 2, 1, 0)
    assert m["vel_excess_ratio"][0] >= 0.25 and m["vel_excess_ratio"][2] >= 0.5 and m["waypoint_updates"] == int((I["wp"] != 0).sum())
    rec.close()
    sol.close()


def test_reset_clears_everything_and_repeats_give_identical_bits(api, torch_cuda):
    """Twenty times the same three replans after lscqp_record_reset: records, distances and points bit for bit; right after a reset the record is
    the empty one whatever was flown before."""
    torch = torch_cuda
    off = np.array([0, 65, 322])
    n = int(off[-1])
    goals = np.random.default_rng(9).uniform(-4, 4, (n, 3))
    sol = _solver(api)
    rec = api.Record(sol, n, off, S, RECORD_DT, TIME_STEP, Z2D, goal_threshold=0.3)
    ref = RR.Record(n, goals, 0.3, TIME_STEP, off)
    rng = np.random.default_rng(21)
    near = np.zeros(n, bool)
    near[:65] = True
    flight = [{k: _dev(torch, v) for k, v in _inputs(api, rng, n, goals, near if r == 1 else None).items()} for r in range(3)]
    first = None
    for rep in range(20):
        rec.reset(goals)
        got, dist = rec.download()
        assert not RR.same_records(got, ref.records()) and not dist.any() and rec.unfinished() == 2 and not rec.points().any()
        for d in flight:
            rec.step_device(d["hdr"], d["x"], d["status"], d["goal_status"], d["sfc_status"], d["valid"], d["in_range"], d["saf"], d["wp"])
        got, dist = rec.download()
        bits = (got.tobytes(), dist.tobytes(), rec.points().tobytes())
        first = first or bits
        assert bits == first, rep
    assert got["finished"].tolist() == [1, 0] and got["replans"].tolist() == [2, 3]
    rec.close()
    sol.close()
