"""Goal LP (reference src/goal_optimizer.cpp): oracle restatement against an independent LP
solver's solutions and the reference log's known answer; the HIP closed form against the oracle."""
import numpy as np
import pytest

from tests import helpers as H


def _case_inputs(O, c):
    cls = O.make_class(M=c["M"], dim=c["dim"], use_sfc=bool(c["use_sfc"]))
    n_obs = len(c["lsc_d"])
    lsc = np.zeros((n_obs, c["M"], 6), O.LSC_DTYPE)
    if n_obs:
        lsc["p"][:, c["M"] - 1, 5] = np.array(c["lsc_p"])
        lsc["nrm"][:, c["M"] - 1, 5] = np.array(c["lsc_nrm"])
        lsc["d"][:, c["M"] - 1, 5] = np.array(c["lsc_d"])
    box = np.zeros(1, O.BOX_DTYPE)
    box["bmin"], box["bmax"] = c["box_min"], c["box_max"]
    return cls, lsc, box


def test_goal_lp_oracle_against_highs_golden(oracle):
    g = H.load_golden("goal_lp")
    n_feas = 0
    for c in g["cases"]:
        cls, lsc, box = _case_inputs(oracle, c)
        a, cc = oracle.goal_rows(cls, c["goal"], c["next_waypoint"], lsc if len(lsc) else None, box[0] if c["use_sfc"] else None)
        assert np.allclose(a, c["rows_a"], rtol=0, atol=1e-15) and np.allclose(cc, c["rows_c"], rtol=0, atol=1e-15)
        st, goal, t = oracle.goal_opt(cls, c["goal"], c["next_waypoint"], lsc if len(lsc) else None, box[0] if c["use_sfc"] else None)
        assert (st == 0) == (c["status"] == 0), (st, c["status"])
        if st == 0:
            n_feas += 1
            assert abs(t - c["t"]) <= 1e-9  # HiGHS run with 1e-10 feasibility tolerances
            gw = np.array(c["goal"]) - np.array(c["next_waypoint"])
            assert np.abs(goal - (gw * c["t"] + np.array(c["next_waypoint"]))).max() <= 1e-8
    assert n_feas >= 100


def test_goal_lp_reference_log_known_answer(oracle):
    """forest10_10, agent 1: waypoint x = 2.5, current goal x = 3.0, the SFC's -x face at 2.55 ->
    GoalOptimizer returns x = 2.55, which is what makes the logged trajectory reproduce (tests/golden/kat_log.json)."""
    cls = oracle.make_class(M=10, dim=2, use_sfc=True)
    box = np.zeros(1, oracle.BOX_DTYPE)
    box["bmin"], box["bmax"] = [2.55, -10, -10], [10, 10, 10]
    st, goal, t = oracle.goal_opt(cls, [3.0, 2.5, 1.0], [2.5, 2.5, 1.0], None, box[0])
    assert st == 0 and abs(goal[0] - 2.55) <= 1e-12 and abs(t - 0.1) <= 1e-12
    kat = H.load_golden("kat_log")
    case = [c for c in kat["cases"] if c["sfc"] is not None][0]
    assert abs(case["goal"][0] - 2.55) <= 1e-6  # the value the QP fixture was generated with


def test_goal_equal_to_waypoint_returns_waypoint(oracle):
    cls = oracle.make_class(M=5, dim=3, use_sfc=False)
    st, goal, t = oracle.goal_opt(cls, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0 + 5e-6])
    assert st == 0 and np.array_equal(goal, [1.0, 2.0, 3.0 + 5e-6])


@pytest.mark.gpu
def test_gpu_goal_lp_matches_oracle_on_golden(api, oracle):
    import torch

    assert torch.cuda.is_available()
    g = H.load_golden("goal_lp")
    by_class = {}
    for c in g["cases"]:
        by_class.setdefault((c["M"], c["dim"], c["use_sfc"]), []).append(c)
    checked = 0
    for (M, dim, use_sfc), cases in by_class.items():
        sol = api.Solver(api.make_desc(M=M, dim=dim, use_sfc=bool(use_sfc)))
        n = len(cases)
        hdr = np.zeros(n, api.HEADER_DTYPE)
        rows, off = [], [0]
        sfc = np.zeros((n, M), api.BOX_DTYPE)
        want = []
        for q, c in enumerate(cases):
            cls, lsc, box = _case_inputs(oracle, c)
            hdr["goal"][q], hdr["next_waypoint"][q] = c["goal"], c["next_waypoint"]
            hdr["n_obs"][q] = len(lsc)
            if len(lsc):
                rows.append(api.pack_rows(lsc).reshape(-1))
            off.append(off[-1] + len(lsc) * M * 6)
            sfc["bmin"][q], sfc["bmax"][q] = box["bmin"][0], box["bmax"][0]
            want.append(oracle.goal_opt(cls, c["goal"], c["next_waypoint"], lsc if len(lsc) else None, box[0] if use_sfc else None))
        rows = np.concatenate(rows) if rows else np.zeros(1, api.ROW_DTYPE)
        out, status = sol.optimize_goal_host(hdr, rows, np.array(off, dtype=np.uint64), sfc if use_sfc else None)
        for q, (st, goal, t) in enumerate(want):
            assert (status[q] == 0) == (st == 0), (q, status[q], st)
            if st == 0:
                # closed form on packed rows (b = d + n.p) vs candidate enumeration on the reference's records: fp64 noise
                assert np.abs(out["goal"][q] - goal).max() <= 1e-9, (q, out["goal"][q], goal)
            else:
                assert np.array_equal(out["goal"][q], hdr["goal"][q])  # untouched
            checked += 1
    assert checked == len(g["cases"])


# ---- constructed cases (tests/post_cases.py): row counts around the 64-lane stride, batch tails, thresholds, finished headers ------
from tests import post_cases as PC  # noqa: E402

_CLASSES = [(3, True), (3, False), (2, True), (2, False)]
_FORMATS = ["f64", "f32"]


def _oracle_goal(oracle, ag, use_sfc, fmt, M=PC.GOAL_M):
    """The oracle on the agent's rows as the row format stores them (reference LSC records with p = 0, so that d = b)."""
    cls = oracle.make_class(M=M, dim=ag["dim"], use_sfc=use_sfc)
    rows = PC.rows_in_format(ag["rows"], fmt)
    lsc = None
    if len(rows):
        lsc = np.zeros((len(rows), M, 6), oracle.LSC_DTYPE)
        lsc["nrm"][:, M - 1, 5], lsc["d"][:, M - 1, 5] = rows[:, :3], rows[:, 3]
    box = np.zeros(1, oracle.BOX_DTYPE)
    box["bmin"][0], box["bmax"][0] = ag["box"]
    return oracle.goal_opt(cls, ag["goal"], ag["w"], lsc, box[0] if use_sfc else None)


def _check_goal_by_construction(ag, fmt, st, goal, tag):
    """(status, goal) against what the case states: t from the binding row as stored, the waypoint, or INFEASIBLE."""
    if ag["kind"] == "infeasible":
        assert st != 0, tag
        return
    assert st == 0, tag
    if ag["kind"] == "waypoint":
        assert np.array_equal(goal, ag["w"]), tag
        return
    t = PC.expected_t(ag, fmt)
    assert abs(t - ag["t"]) <= (1e-6 if fmt == "f32" else 1e-12), (tag, t)  # float32 rows move a bound by 2^-24 of its terms
    # fp64 on both sides, a handful of operations on values of order 1 (contraction may differ): a few 1e-16
    assert np.abs(goal - ((ag["goal"] - ag["w"]) * t + ag["w"])).max() <= 1e-12, (tag, goal, t)


def _goal_cases(dim, use_sfc):
    return PC.goal_rowcount_agents(dim, use_sfc) + PC.goal_edge_agents(dim)


@pytest.mark.parametrize("dim,use_sfc", _CLASSES)
def test_goal_constructed_cases_on_oracle(oracle, dim, use_sfc):
    cases = _goal_cases(dim, use_sfc) + PC.goal_ragged_agents(dim, use_sfc)
    assert {c["kind"] for c in cases} == {"t", "infeasible", "waypoint"}
    for ag in cases:
        for fmt in _FORMATS:
            st, goal, _ = _oracle_goal(oracle, ag, use_sfc, fmt)
            _check_goal_by_construction(ag, fmt, st, goal, (ag["name"], fmt))


@pytest.mark.parametrize("dim,use_sfc", [(3, True), (2, False)])
def test_goal_finished_headers_on_oracle(oracle, dim, use_sfc):
    """terminal_segments by construction = the oracle's and the numpy restatement's, on the float32 goal the chain keeps."""
    M = PC.GOAL_M
    agents, want_ts = PC.goal_fin_agents(dim)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=use_sfc)
    assert set(want_ts) == set(range(1, M)) and (np.array([a["kind"] for a in agents]) == "infeasible").sum() == 2
    for ag, ts in zip(agents, want_ts):
        st, goal, _ = _oracle_goal(oracle, ag, use_sfc, "f64")
        _check_goal_by_construction(ag, "f64", st, goal, ag["name"])
        g32 = PC.f32(goal if st == 0 else ag["goal"])
        oa = oracle.make_agent(ag["p0"], g32, nominal_velocity=ag["nominal_velocity"])
        assert oracle.terminal_segments(cls, oa) == ts == PC.terminal_segments_np(g32, ag["p0"], ag["nominal_velocity"], M, PC.DT), ag["name"]


def _goal_device(api, agents, dim, use_sfc, fmt, n=None, fin_dt=None, M=PC.GOAL_M):
    """One launch of the goal LP over agents[:n].  Every row and box the kernel must NOT read (all but (obstacle, M - 1, 5) and the last
    segment's box) would make the LP infeasible; one guard header and one status word sit behind the batch.
    Returns (hdr in, hdr out, status), the guards included."""
    import torch

    n = len(agents) if n is None else n
    agents = agents[:n]
    sol = api.Solver(api.make_desc(M=M, dim=dim, use_sfc=use_sfc, row_format=api.ROWS_F32 if fmt == "f32" else api.ROWS_F64))
    hdr = np.zeros(n + 1, api.HEADER_DTYPE)
    hdr.view(np.uint8)[-api.HEADER_DTYPE.itemsize:] = 0xA5
    sfc = np.zeros((n, M), api.BOX_DTYPE)
    sfc["bmin"], sfc["bmax"] = 1e3, 1e3  # a box no point of the segment g - w lies in
    rows, off = [], [0]
    for q, ag in enumerate(agents):
        hdr["goal"][q], hdr["next_waypoint"][q], hdr["p0"][q] = ag["goal"], ag["w"], ag["p0"]
        hdr["nominal_velocity"][q], hdr["n_obs"][q], hdr["terminal_segments"][q] = ag["nominal_velocity"], len(ag["rows"]), -5
        sfc["bmin"][q, M - 1], sfc["bmax"][q, M - 1] = ag["box"]
        r = np.zeros((len(ag["rows"]), M, 6), api.ROW_DTYPE)
        r["nx"], r["b"] = -np.sign(ag["goal"][0] - ag["w"][0]), 1e3  # t <= a negative number
        for f, col in zip(("nx", "ny", "nz", "b"), ag["rows"].T):
            r[f][:, M - 1, 5] = col
        rows.append(r.reshape(-1))
        off.append(off[-1] + r.size)
    rows = sol.rows_in_format(np.concatenate(rows + [np.zeros(1, api.ROW_DTYPE)]))
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_hdr, d_status = up(hdr), torch.full((n + 1,), -77, dtype=torch.int32, device=dev)
    args = (n, d_hdr, up(rows), up(np.array(off, dtype=np.uint64)), up(sfc) if use_sfc else None, d_status)
    if fin_dt is None:
        sol.optimize_goal_device(*args)
    else:
        sol.optimize_goal_fin_device(*args, fin_dt)
    torch.cuda.synchronize()
    return hdr, d_hdr.cpu().numpy().view(api.HEADER_DTYPE), d_status.cpu().numpy()


def _check_goal_device(oracle, agents, use_sfc, fmt, hdr, out, status):
    n = len(agents)
    for q, ag in enumerate(agents):
        tag = (q, ag["name"], fmt)
        st, goal, _ = _oracle_goal(oracle, ag, use_sfc, fmt)
        assert status[q] == (0 if st == 0 else 1), (tag, status[q], st)
        _check_goal_by_construction(ag, fmt, int(status[q]), out["goal"][q], tag)
        if st == 0:
            assert np.abs(out["goal"][q] - goal).max() <= 1e-12, (tag, out["goal"][q], goal)
        else:
            assert out["goal"][q].tobytes() == hdr["goal"][q].tobytes(), tag  # keeps its bits
        assert out["terminal_segments"][q] == -5, tag  # not this entry's to write
    # nothing is written beyond n: the guard header and the status word behind the batch
    assert out[n:].tobytes() == hdr[n:].tobytes() and status[n] == -77
    for f in out.dtype.names:  # every other field of the headers keeps its bits
        if f not in ("goal", "terminal_segments"):
            assert np.ascontiguousarray(out[f][:n]).tobytes() == np.ascontiguousarray(hdr[f][:n]).tobytes(), f


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", _FORMATS)
@pytest.mark.parametrize("dim,use_sfc", _CLASSES)
def test_gpu_goal_constructed_cases(api, oracle, dim, use_sfc, fmt):
    """Row counts on both sides of 64 and 128 with the binding bound at row 0, 63, 64 and last, a binding upper bound behind row 64,
    a == 0 rows, the short-normal skip, the variable's cap and the |g - w| threshold: the device against the oracle and the stated t."""
    agents = _goal_cases(dim, use_sfc)
    hdr, out, status = _goal_device(api, agents, dim, use_sfc, fmt)
    _check_goal_device(oracle, agents, use_sfc, fmt, hdr, out, status)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("dim,use_sfc", [(3, True), (2, False)])
def test_gpu_goal_batch_tails(api, oracle, dim, use_sfc, n):
    """Four agents per workgroup: batches that end inside one, ragged row counts, zero-row agents; nothing written beyond n."""
    agents = PC.goal_ragged_agents(dim, use_sfc)
    assert len(agents) == 9 and min(len(a["rows"]) for a in agents) == 0
    for fmt in _FORMATS:
        hdr, out, status = _goal_device(api, agents, dim, use_sfc, fmt, n=n)
        _check_goal_device(oracle, agents[:n], use_sfc, fmt, hdr, out, status)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", _FORMATS)
@pytest.mark.parametrize("dim,use_sfc", [(3, True), (2, False)])
def test_gpu_goal_finished_headers(api, oracle, dim, use_sfc, fmt):
    """The chain's entry (fin_dt = dt): the goal is left as a point3d and terminal_segments comes from it -- value for value what
    finalize_goal_kernel leaves: float32(oracle goal) (float32(OLD goal) where the LP is infeasible) and orc_terminal_segments on it."""
    M = PC.GOAL_M
    agents, want_ts = PC.goal_fin_agents(dim)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=use_sfc)
    hdr, out, status = _goal_device(api, agents, dim, use_sfc, fmt, fin_dt=PC.DT)
    n = len(agents)
    for q, ag in enumerate(agents):
        tag = (q, ag["name"], fmt)
        st, goal, _ = _oracle_goal(oracle, ag, use_sfc, fmt)
        assert (status[q] == 0) == (st == 0) == (ag["kind"] == "t"), tag
        got = out["goal"][q]
        assert np.array_equal(got, PC.f32(got)), tag  # float32 values
        g32 = np.float32(goal if st == 0 else ag["goal"])
        # one float32 ulp where the two fp64 goals differ in their last bits and straddle a rounding boundary; none for the old goal
        assert (np.abs(got - g32.astype(np.float64)) <= (np.spacing(np.abs(g32)).astype(np.float64) if st == 0 else 0.0)).all(), (tag, got, g32)
        oa = oracle.make_agent(ag["p0"], got, nominal_velocity=ag["nominal_velocity"])
        assert out["terminal_segments"][q] == oracle.terminal_segments(cls, oa) == want_ts[q], (tag, out["terminal_segments"][q], want_ts[q])
    assert out[n:].tobytes() == hdr[n:].tobytes() and status[n] == -77
