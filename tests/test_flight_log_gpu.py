"""The flight log on the device (include/lscqp.h, "the flight log"; csrc/lscrecord.hip: flight_log_kernel): the stand-alone record entries on
constructed inputs -- no QP is solved -- against the numpy restatement (tests/flight_log_reference.py).  Positions are compared with the
record's own points bit for bit, velocities and accelerations with a float64 evaluation to one float32 ulp, and WHERE the kernel wrote is
checked against a sentinel that fills all three raw buffers beforehand."""
import numpy as np
import pytest

from tests import flight_log_reference as FL

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)  # both sides of a wavefront and of a 256-thread tile; with S = 3 a tile straddles agents
OFF = np.concatenate([[0], np.cumsum(SIZES)])
N = int(OFF[-1])
TIME_STEP = 0.2
SENTINEL = 0x7FC12345  # (a NaN's bits as float32: compared as int32)
# (M, dim, dt, z_2d).  dt = 0.25 is dyadic, so a sample at k * dt lies EXACTLY on a segment boundary in the search's own arithmetic
SHAPES = {"M5_dim3": (5, 3, 0.25, 1.0), "M10_dim2": (10, 2, 0.25, 0.6), "M5_dim2_dt02": (5, 2, 0.2, 0.6)}
# (shape, S, record_time_step): sample 1 on a boundary and sample 2 beyond the horizon (M5: 0.75, 1.5 > 1.25; M10: 1.25, 2.5 = M dt); sample 1
# beyond it; every sample inside a segment; the launch files' 0.1 at dt = 0.2
CASES = [("M5_dim3", 1, 0.75), ("M5_dim3", 2, 0.75), ("M5_dim3", 2, 1.5), ("M5_dim3", 3, 0.75), ("M5_dim3", 3, 0.1),
         ("M10_dim2", 1, 1.25), ("M10_dim2", 2, 1.25), ("M10_dim2", 3, 1.25), ("M10_dim2", 3, 0.3), ("M5_dim2_dt02", 2, 0.1), ("M5_dim2_dt02", 3, 0.1)]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _inputs(api, rng, nv, goals, near=None):
    """One replan's inputs for N agents: random plans and figures over every status value; `near`: the agents that start AT their goals."""
    hdr = np.zeros(N, api.HEADER_DTYPE)
    hdr["p0"] = goals + rng.uniform(1.0, 2.0, (N, 3))
    if near is not None:
        hdr["p0"][near] = goals[near]
    hdr["n_obs"] = rng.integers(0, 6, N)
    saf = np.zeros(N, api.SAFETY_DTYPE)
    saf["safety_ratio"] = rng.uniform(1.0, 3.0, N)
    saf["closest_agent"] = rng.integers(0, N, N)
    ints = dict(status=rng.integers(0, 5, N), goal_status=rng.integers(0, 3, N), sfc_status=rng.integers(0, 2, N), valid=rng.integers(0, 2, N),
                in_range=rng.integers(0, 9, N), wp=rng.integers(0, 2, N))
    return dict(x=rng.uniform(-4, 4, (N, nv)), hdr=hdr, saf=saf, **{k: v.astype(np.int32) for k, v in ints.items()})


def _step(torch, rec, I, with_wp=True):
    d = {k: _dev(torch, v) for k, v in I.items()}
    rec.step_device(d["hdr"], d["x"], d["status"], d["goal_status"], d["sfc_status"], d["valid"], d["in_range"], d["saf"], d["wp"] if with_wp else None)
    return rec.points()  # (waits for the device)


def _record(api, shape, S, rts, threshold=0.5):
    M, dim, dt, z = SHAPES[shape]
    sol = api.Solver(api.make_desc(M=M, dim=dim, dt=dt))
    return sol, api.Record(sol, N, OFF, S, rts, TIME_STEP, z, goal_threshold=threshold)


def _near(k):
    near = np.zeros(N, bool)
    near[OFF[k]:OFF[k + 1]] = True
    return near


def _raw(torch, rec):
    """The three raw buffers as int32 numpy arrays (an empty one where the log has no obstacle columns)."""
    torch.cuda.synchronize()
    out = []
    for which in (0, 1, 2):
        t = rec.log_tensor(which)
        out.append(np.zeros(0, np.int32) if t is None else t.view(torch.int32).cpu().numpy())
    return out


def _fill(torch, rec):
    for which in (0, 1, 2):
        t = rec.log_tensor(which)
        if t is not None:
            t.view(torch.int32).fill_(SENTINEL)
    torch.cuda.synchronize()


def _bars(want, dt):
    """One float32 ulp of the float64 value, + the 1e-14 floor of tests/test_record_gpu.py for positions scaled by the factors the derivative
    control points carry: 5/dt for velocities, 20/dt^2 for accelerations (derived, not measured)."""
    floor = np.repeat([1e-14, 1e-14 * 5 / dt, 1e-14 * 20 / dt ** 2], 3)
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + floor


@pytest.mark.parametrize("shape,S,rts", CASES, ids=["%s-S%d-rts%g" % c for c in CASES])
def test_states_and_flags_equal_the_restatement(api, torch_cuda, shape, S, rts):
    """Three replans of random plans, capacity 3, five missions of 1 .. 257 agents.  Per replan and mission: the log's positions are the
    record's points bit for bit; positions, velocities and accelerations lie within one float32 ulp of the float64 restatement; in 2-D
    pz = float32(z_2d) and vz = az = 0 exactly; the flags word is the restatement's.  After the flight the per-bit sums of a mission's rows are
    the record's five counters."""
    torch = torch_cuda
    M, dim, dt, z = SHAPES[shape]
    rng = np.random.default_rng(41)
    goals = rng.uniform(-4, 4, (N, 3))
    sol, rec = _record(api, shape, S, rts)
    rec.reset(goals)
    rec.set_log(3)
    flown = []
    for r in range(3):
        I = _inputs(api, rng, dim * M * 6, goals)
        flown.append((I, _step(torch, rec, I)))
    rows, over = rec.log_rows()
    assert rows.tolist() == [3] * 5 and over.tolist() == [0] * 5
    got, _ = rec.download()
    for k in range(5):
        lo, hi = OFF[k], OFF[k + 1]
        st, fl, ob = rec.log(k)
        assert st.shape == (3, SIZES[k], S, 9) and fl.shape == (3, SIZES[k]) and ob.shape == (3, 0, 4)
        for r, (I, pts) in enumerate(flown):
            assert st[r, :, :, 0:3].tobytes() == pts[lo:hi].tobytes(), (k, r)
            want = FL.states_f64(I["x"][lo:hi], M, dim, dt, S, rts, z)
            assert (np.abs(st[r].astype(np.float64) - want) <= _bars(want, dt)).all(), (k, r)
            if dim == 2:
                assert (st[r, :, :, 2] == np.float32(z)).all() and not st[r, :, :, 5].any() and not st[r, :, :, 8].any()
            word = FL.flags_word(I["status"][lo:hi], I["valid"][lo:hi], I["goal_status"][lo:hi], I["sfc_status"][lo:hi], I["wp"][lo:hi])
            assert np.array_equal(fl[r], word), (k, r)
        for bit, field in enumerate(FL.FLAG_FIELDS):
            assert int(((fl >> bit) & 1).sum()) == int(got[field][k]), (k, field)
    assert got["qp_failed"].sum() > 0 and got["waypoint_updates"].sum() > 0
    st, fl, _ = rec.log(4, first_replan=1, n_replans=1)  # a part of a mission's rows
    assert st.tobytes() == rec.log(4)[0][1:2].tobytes() and fl.tobytes() == rec.log(4)[1][1:2].tobytes()
    rec.close()
    sol.close()


@pytest.mark.parametrize("S", [1, 2, 3])
def test_only_the_rows_of_live_missions_below_the_capacity_are_written(api, torch_cuda, S):
    """All three raw buffers filled with a sentinel; 5 replans of distinct random plans at capacity 3, with three obstacle columns whose table
    is rewritten before every replan; mission 1 finishes at replan 1.  Rows 0-2 of the live missions hold replans 0-2 -- the log ran before
    the record's increment -- mission 1 holds rows 0-1 only, the obstacle rows are the table of their replan, and EVERY OTHER BYTE is still the
    sentinel.  log_rows gives (3, 2, 3, 3, 3), overflowed (1, 0, 1, 1, 1).  No step device buffer for the waypoint bit: it is never set."""
    torch = torch_cuda
    M, dim, dt, z = SHAPES["M5_dim3"]
    rts, Cap, nd = 0.75, 3, 3
    rng = np.random.default_rng(43)
    goals = rng.uniform(-4, 4, (N, 3))
    sol, rec = _record(api, "M5_dim3", S, rts)
    rec.reset(goals)
    rec.set_log(Cap, nd)
    table = np.zeros(nd, api.OBSTACLE_DTYPE)
    d_table = _dev(torch, table)
    rec.log_obstacles(d_table)
    _fill(torch, rec)
    flown = []
    for r in range(5):
        table["position"], table["radius"] = rng.uniform(-4, 4, (nd, 3)), rng.uniform(0.1, 0.5, nd)
        d_table.copy_(_dev(torch, table))
        I = _inputs(api, rng, dim * M * 6, goals, _near(1) if r == 1 else None)
        flown.append((I, _step(torch, rec, I, with_wp=False), table.copy()))
    rows, over = rec.log_rows()
    assert rows.tolist() == [3, 2, 3, 3, 3] and over.tolist() == [1, 0, 1, 1, 1]
    assert rec.download()[0]["replans"].tolist() == [5, 2, 5, 5, 5]
    raw = _raw(torch, rec)
    assert [a.size for a in raw] == list(FL.sizes(OFF, S, Cap, nd))
    written = [np.zeros(a.size, bool) for a in raw]
    for k in range(5):
        val = FL.mission_views(OFF, k, S, Cap, nd, raw[0].view(np.float32), raw[1], raw[2].view(np.float32))
        msk = FL.mission_views(OFF, k, S, Cap, nd, *written)
        lo, hi = OFF[k], OFF[k + 1]
        for r in range(int(rows[k])):
            I, pts, tab = flown[r]
            for m in msk:
                m[r] = True
            assert val[0][r, :, :, 0:3].tobytes() == pts[lo:hi].tobytes(), (k, r)
            want = FL.states_f64(I["x"][lo:hi], M, dim, dt, S, rts, z)
            assert (np.abs(val[0][r].astype(np.float64) - want) <= _bars(want, dt)).all(), (k, r)
            assert np.array_equal(val[1][r], FL.flags_word(I["status"][lo:hi], I["valid"][lo:hi], I["goal_status"][lo:hi], I["sfc_status"][lo:hi]))
            assert np.array_equal(val[2][r, :, 0:3], tab["position"].astype(np.float32)) and np.array_equal(val[2][r, :, 3], tab["radius"].astype(np.float32))
    for a, w in zip(raw, written):
        assert w.any() and not w.all()
        assert (a[~w] == SENTINEL).all()
    # a NULL table: the states are logged, the obstacle entries are not
    rec.reset(goals)
    rec.log_obstacles(None)
    _fill(torch, rec)
    _step(torch, rec, flown[0][0])
    raw = _raw(torch, rec)
    assert (raw[2] == SENTINEL).all() and (raw[0] != SENTINEL).any() and rec.log_rows()[0].tolist() == [1] * 5
    rec.close()
    sol.close()


def test_the_record_is_untouched_by_its_log(api, torch_cuda):
    """The same four replans (mission 2 finishes at replan 2) into a record with a log and one without: records, distances and points are
    byte-identical after every replan."""
    torch = torch_cuda
    M, dim, dt, z = SHAPES["M10_dim2"]
    rng = np.random.default_rng(47)
    goals = rng.uniform(-4, 4, (N, 3))
    sol, plain = _record(api, "M10_dim2", 2, 0.1)
    sol2, logged = _record(api, "M10_dim2", 2, 0.1)
    logged.set_log(2, 1)  # (an overflowing one, with obstacle columns and no table)
    for rec in (plain, logged):
        rec.reset(goals)
    for r in range(4):
        I = _inputs(api, rng, dim * M * 6, goals, _near(2) if r == 2 else None)
        pa, pb = _step(torch, plain, I), _step(torch, logged, I)
        (ra, da), (rb, db) = plain.download(), logged.download()
        assert ra.tobytes() == rb.tobytes() and da.tobytes() == db.tobytes() and pa.tobytes() == pb.tobytes(), r
        assert plain.unfinished() == logged.unfinished()
    assert rb["finished"].tolist() == [0, 0, 1, 0, 0] and logged.log_rows()[1].tolist() == [1, 1, 1, 1, 1]
    for rec, s in ((plain, sol), (logged, sol2)):
        rec.close()
        s.close()


def test_after_a_reset_the_same_replans_give_the_same_rows(api, torch_cuda):
    """lscqp_record_reset clears nothing of the log and the rows restart at 0: the same three replans after a reset -- the buffers overwritten
    with the sentinel in between -- reproduce the first three rows bit for bit."""
    torch = torch_cuda
    M, dim, dt, z = SHAPES["M5_dim2_dt02"]
    rng = np.random.default_rng(53)
    goals = rng.uniform(-4, 4, (N, 3))
    sol, rec = _record(api, "M5_dim2_dt02", 3, 0.1)
    rec.set_log(4)
    flight = [_inputs(api, rng, dim * M * 6, goals, _near(3) if r == 1 else None) for r in range(3)]
    first = None
    for rep in range(2):
        rec.reset(goals)
        assert rec.log_rows()[0].tolist() == [0] * 5
        if rep == 0:
            before = _raw(torch, rec)
            assert not before[0].any() and not before[1].any()  # (zeroed once, when it was attached)
        _fill(torch, rec)
        for I in flight:
            _step(torch, rec, I)
        assert rec.log_rows()[0].tolist() == [3, 3, 3, 2, 3]
        bits = tuple(rec.log(k)[i].tobytes() for k in range(5) for i in (0, 1))
        first = first or bits
        assert bits == first
        assert (_raw(torch, rec)[0] == SENTINEL).any()  # (row 3, and mission 3's row 2)
    rec.close()
    sol.close()


def test_removal_and_refused_downloads(api, torch_cuda):
    """set_log(0) removes the log: the log entries are refused with the cause named and a step enqueues the record alone.  A download past a
    mission's rows, of an unknown mission or of a negative range is LSCQP_ERR_INVALID_ARGUMENT; an empty range is not."""
    torch = torch_cuda
    M, dim, dt, z = SHAPES["M5_dim3"]
    rng = np.random.default_rng(59)
    goals = rng.uniform(-4, 4, (N, 3))
    sol, rec = _record(api, "M5_dim3", 2, 0.1)
    rec.reset(goals)
    with pytest.raises(api.LscqpError, match="no log") as e:
        rec.log_rows()
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    with pytest.raises(api.LscqpError, match="no log"):
        rec.log_obstacles(None)
    rec.set_log(2)
    with pytest.raises(api.LscqpError, match="no obstacle columns"):
        rec.log_obstacles(_dev(torch, np.zeros(1, api.OBSTACLE_DTYPE)))
    I = _inputs(api, rng, dim * M * 6, goals)
    _step(torch, rec, I)
    assert rec.log(0)[0].shape == (1, 1, 2, 9) and rec.log(0, 1, 0)[0].shape == (0, 1, 2, 9)
    for bad in ((0, 0, 2), (0, 1, 1), (5, 0, 1), (-1, 0, 1), (0, -1, 1)):
        with pytest.raises(api.LscqpError) as e:
            rec.log(*bad)
        assert e.value.code == api.ERR_INVALID_ARGUMENT, bad
    with pytest.raises(api.LscqpError, match="exceed the mission's 1 logged rows"):
        rec.log(4, 0, 2)
    with pytest.raises(api.LscqpError, match="max_replans"):
        rec.set_log(-1)
    assert rec.log_rows()[0].tolist() == [1] * 5  # (the refused call left the log as it was)
    rec.set_log(0)
    for call in (rec.log_rows, lambda: rec.log(0, 0, 0), lambda: rec.log_tensor(0)):
        with pytest.raises(api.LscqpError, match="no log"):
            call()
    _step(torch, rec, I)
    assert rec.download()[0]["replans"].tolist() == [2] * 5
    rec.close()
    sol.close()
