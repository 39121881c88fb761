"""The fused phase's latency text built without machine-level hoisting in front of its loop of steps, and its wavefront reductions on
DPP steps without identity moves (lsc_dr_planner_amd/build.py: fused_flags; csrc/lscqp_das.hpp: wave_argmin_ror, wave_reduce3_zero,
wave_reduce1_zero; NOTES section 45) -- on the inputs at which set-up that now stands inside an arm (the polish, a leaving row, the
decision with rows held, the hand-over with the arguments it reads late, the proof), or a reduction's lane, can go wrong.

Small batches (at most 8 instances) of the two fused shapes that run the latency text, M5 in 3-D and M10 in 2-D, each through the four
forms of tests/test_das_prologue.py: the fused launch (the new machine code) against the two launches and the one- and two-wavefront
forms (the throughput text: lscqp::wave_reduce3 and wave_argmin as they were, the default optimiser).  Every form must return the same
bytes in x, obj, status and info; every instance expected OPTIMAL is finished by the phase in the restatement's step count and held to
the polished CPU oracle at 1e-8 m / 1e-8 relative (tests/test_das_step_path.py: every_form).  The builders are those of
tests/das_cases.py and of the step-path, round-trip and row-register files, with their premises asserted on the CPU by the restatement's
trace; the two builders of this file say theirs.  LSC row j = 6 M o + 6 m + i is thread j mod 256's: lane j mod 64 of wavefront
(j mod 256) div 64."""
import numpy as np
import pytest

from tests import das_cases as DC
from tests import test_das_prologue as PR
from tests import test_das_round_trips as RT
from tests import test_das_row_registers as RR
from tests import test_das_step_path as SP
from tests.test_das_prologue import FORMS, SHAPE_IDS, SHAPES, _device_call, _same

pytestmark = pytest.mark.gpu

OPTIMAL, INFEASIBLE, HANDED = SP.OPTIMAL, SP.INFEASIBLE, SP.HANDED
T = RT.T
FIELDS, NO_INFO = ("x", "obj", "status", "info"), ("x", "obj", "status")
LANES = [(0, 15), (16, 31), (32, 63)]  # the first and the last lane of the DPP rows: lane 0 has no source in any row_shr step


def _cap(M):
    return max(SP.OBSTACLES[M])


def _forms(api, torch, b, knobs=None, **kw):
    """the batch through the four forms with the entry's optional pointers chosen by the caller: the same bytes from each"""
    res = [RT._call(api, torch, b, dict(k, **(knobs or {})), **kw) for _, k in FORMS]
    fields = FIELDS if kw.get("info", True) else NO_INFO
    for (name, _), r in zip(FORMS[1:], res[1:]):
        assert RT._same_fields(r, res[0], fields), (name, r["status"], res[0]["status"])
    return res[0]


# ---- a quiet instance beside a stepping one; one step with k == 0; a permuted order; no info_out ----------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_quiet_instance_beside_a_stepping_one(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    step = SP.batch(("stepper",) + shape, lambda: SP.plane_case(oracle, spec, _cap(M), [(_cap(M) - 1, M // 2, [-1.0, 0.0, 0.0], 0.6)], seed=3, name="stepper"))
    quiet = SP.batch(("quiet",) + shape, lambda: SP.quiet_case(oracle, spec))
    b = SP.batch(("ep beside",) + shape, lambda: SP.make_batch(api, oracle, spec, [quiet, step, quiet]))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert list(G["info"]["iterations"]) == [0, 1, 0]
    assert G["x"][0].tobytes() == G["x"][2].tobytes() and G["info"][0].tobytes() == G["info"][2].tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_one_step_from_no_row_held_in_a_permuted_order_and_without_info_out(api, oracle, torch_cuda, shape):
    """every instance takes ONE step with k == 0 (the first-row decision); then the same launch in a permuted order, and with info_out
    absent: nothing but the record depends on it"""
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("tails",) + shape, lambda: SP.make_batch(api, oracle, spec, SP.tail_cases(oracle, spec, PR.capacity_of(api, M, dim))))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] == 1).all(), G["info"]["iterations"]
    n = len(b.hdr)
    perm = [(3 * q + 2) % n for q in range(n)]
    assert sorted(perm) == list(range(n)) and perm != list(range(n))
    R = _forms(api, torch_cuda, b, order=perm)
    N = _forms(api, torch_cuda, b, order=perm, info=False)
    assert RT._same_fields(R, G, FIELDS) and RT._same_fields(N, G, NO_INFO)


# ---- two and three rows held (the decision for k > 0); the two budgets' hand-overs, with and without x_init -------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_two_and_three_rows_held_and_both_budgets_hand_over_with_and_without_x_init(api, oracle, torch_cuda, shape):
    """one, two and three corridor faces across the way: the general decision with one and two rows held.  Then das_kmax 1 and
    das_steps 1: the second candidate ends the phase, hand_over writes the start -- x_init where the call has one, the header's p0
    where not -- and the interior-point instance behind it in the same launch reads x_init, x_out, status_out and info_out"""
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")

    def make():
        fam = SP.family_and_held_cases(oracle, spec)
        return SP.make_batch(api, oracle, spec, [fam[0], fam[4], fam[5]])

    b = SP.batch(("budgets",) + shape, make)
    g = [SP.restated(oracle, c) for c in b.cases]
    assert [x["steps"] for x in g] == [1, 2, 3] and [x["peak"] for x in g][1:] == [2, 3]
    b.expect = [OPTIMAL] * 3
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert list(G["info"]["iterations"]) == [1, 2, 3]
    # (a previous plan: the oracle's optimum, a millimetre off)
    xi = np.stack([b.ref[q][0].reshape(-1) for q in range(3)]) + 1e-3 * np.random.RandomState(7).randn(*G["x"].shape)
    try:
        for knobs in (dict(das_kmax=1), dict(das_steps=1)):
            b.expect = [OPTIMAL, HANDED, HANDED]
            H = SP.every_form(api, oracle, torch_cuda, b, knobs=knobs)  # (without x_init)
            W = _forms(api, torch_cuda, b, knobs=knobs, x_init=xi)
            assert (W["status"] == api.STATUS_OPTIMAL).all(), W["status"]
            assert RT._same_fields({f: W[f][:1] for f in W}, {f: H[f][:1] for f in H}, FIELDS)  # (what the phase finishes does not read x_init)
            for q in (1, 2):  # the interior-point pass's, started somewhere else: its own bar against the oracle
                assert not (W["info"]["flags"][q] & api.INFO_ACTIVE_SET)
                assert np.abs(W["x"][q] - b.ref[q][0]).max() <= SP.IP_X_TOL, (knobs, q)
    finally:
        b.expect = [OPTIMAL] * 3


# ---- a row that leaves and rejoins; the proof with rows held; an empty interval -------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_row_leaves_and_rejoins_beside_a_proof_of_infeasibility_and_an_empty_interval(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rr rejoin",) + shape, lambda: SP.make_batch(api, oracle, spec, [RR.rejoining_case(oracle, spec), SP.infeasible_case(oracle, spec)],
                                                             expect=[OPTIMAL, INFEASIBLE]))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert G["info"]["iterations"][0] >= 3  # (joins, leaves -- kind 2, the descriptors' shuffle and the factor's downdate -- and joins again)
    assert G["obj"][1] == 0.0 and np.array_equal(G["x"][1].reshape(dim, -1), np.repeat(b.hdr["p0"][1][:dim, None], 6 * M, axis=1))  # (infeasible_out: the start)
    xi = np.random.RandomState(8).uniform(-0.5, 0.5, G["x"].shape)
    W = _forms(api, torch_cuda, b, x_init=xi)
    assert np.array_equal(W["status"], G["status"]) and W["x"][1].tobytes() == xi[1].tobytes() and W["x"][0].tobytes() == G["x"][0].tobytes()
    e = PR.batch(("rt empty",) + shape, RT.empty_batch, api, oracle, M, dim)
    E = PR.every_form(api, oracle, torch_cuda, e)
    assert list(E["status"]) == [api.STATUS_INFEASIBLE] * 3 + [api.STATUS_OPTIMAL]


# ---- an instance over the launch's cap ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_an_instance_over_the_cap_is_handed_over_before_its_rows_are_read(api, oracle, torch_cuda, shape):
    M, dim = shape
    cap = PR.capacity_of(api, M, dim)
    b = PR.batch(("mixed",) + shape, PR.mixed_counts, api, oracle, M, dim, cap)
    G = PR.every_form(api, oracle, torch_cuda, b)
    q = b.expect.index(PR.CAPACITY)
    xi = np.random.RandomState(3).randn(*G["x"].shape)
    W = _forms(api, torch_cuda, b, x_init=xi)
    ok = np.arange(len(b.hdr)) != q
    assert np.array_equal(W["status"], G["status"]) and W["status"][q] == api.STATUS_CAPACITY
    assert RT._same_fields({f: W[f][ok] for f in W}, {f: G[f][ok] for f in G}, FIELDS)
    assert np.isfinite(W["x"]).all()  # (the NaN between the instances' rows reached nobody)


# ---- a NaN in a live row ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_nan_in_a_live_row_is_numeric_in_every_form(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")

    def make():
        b = SP.make_batch(api, oracle, spec, [SP.quiet_case(oracle, spec)] + RT.wave_cases(oracle, spec)[1:3])
        b.rows = b.rows.copy()
        j = int(b.off[2]) + RT.WAVE_SLOTS[M][2] * 6 * M + 6 * (M // 2) + 4  # a live row of the third instance, in wavefront 2
        assert np.isfinite(b.rows["b"][j]) and b.rows["nx"][j] != 0.0
        b.rows["b"][j] = np.nan
        return b

    b = SP.batch(("ep nan",) + shape, make)
    res = [_device_call(api, torch_cuda, b, knobs) for _, knobs in FORMS]
    assert all(_same(r, res[0]) for r in res[1:])
    assert list(res[0]["status"]) == [api.STATUS_OPTIMAL, api.STATUS_OPTIMAL, api.STATUS_NUMERIC], res[0]["status"]


# ---- wave_argmin: the minimum in the first and the last lane of every DPP row of every wavefront ---------------------------------------------
def _cut_agent(spec):
    """along axis 0 only: the free trajectory's control points on the other axes are 0 relative to the start, exactly, on the device too
    (c_u = cfix - c1 U1 - c2 U2 + 2 w_t (goal - p0) G1 with v0 = a0 = goal - p0 = 0 on that axis)"""
    p0 = DC._p0(spec)
    goal = p0 + np.array([1.0, 0.0, 0.0])
    return dict(p0=p0, v0=np.array([0.2, 0.0, 0.0]), a0=np.zeros(3), goal=goal, next_waypoint=goal.copy(), nominal_velocity=1.0, radius=0.15)


def row_case(O, spec, cuts, seed, name):
    """a full instance (the cap's obstacles) whose every row stays a metre clear of the free trajectory (SP.plane_case's filler), but
    for `cuts`: [(row id j, normal, depth)] -- the ONE row j asks the control point it names to move `depth` metres along the normal"""
    M, dim = spec["M"], spec["dim"]
    a = _cut_agent(spec)
    n_obs = _cap(M)
    p0 = np.asarray(a["p0"], float)
    c = DC._free(O, spec, **a) + p0[:dim, None, None]
    L = np.zeros((n_obs, M, 6), O.LSC_DTYPE)
    rng = np.random.RandomState(seed)
    for oi in range(n_obs):
        for m in range(M):
            n = rng.randn(3)
            n[2] = n[2] if dim == 3 else 0.0
            n /= np.linalg.norm(n)
            vals = np.einsum("k,ki->i", n[:dim], c[:, m])
            L["nrm"][oi, m] = n
            L["d"][oi, m] = float(np.float32(min(vals.min(), float(n[:dim] @ p0[:dim])) - 1.0))
    for (j, nrm, depth) in cuts:
        o, m, i = j // (6 * M), (j % (6 * M)) // 6, j % 6
        n = np.asarray(nrm, float)
        L["nrm"][o, m, i] = n
        L["d"][o, m, i] = float(np.float32(float(n[:dim] @ c[:, m, i]) + depth))
    return DC.Case(name, spec, O.make_agent(n_obs=n_obs, **dict(DC.LOOSE, **a)), lsc=L)


def _row_of_thread(M, t):
    """the lowest LSC row of thread t that is no row of segment 0 (its first control points are dropped or fixed)"""
    for u in range(3):
        j = t + T * u
        if j < 6 * M * _cap(M) and j % (6 * M) >= 6:
            return j
    raise AssertionError(t)


def lane_cases(O, spec, lanes):
    out = []
    for w in range(4):
        for lane in lanes:
            j = _row_of_thread(spec["M"], 64 * w + lane)
            c = row_case(O, spec, [(j, RT.OBLIQUE[spec["dim"]], 0.05)], seed=300 + j, name="minimum_in_lane_%d_of_wavefront_%d" % (lane, w))
            g, tr = RT._traced(O, c)
            assert g["status"] == "optimal" and g["steps"] >= 1 and tr[0]["family"] == "lsc" and tr[0]["row"] == j, (c, j, tr[:1])
            assert ((j % T) >> 6, j % 64) == (w, lane)
            out.append(c)
    return out


@pytest.mark.parametrize("lanes", LANES, ids=["lanes_%d_%d" % l for l in LANES])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_minimum_in_the_first_and_the_last_lane_of_each_dpp_row_of_each_wavefront(api, oracle, torch_cuda, shape, lanes):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("ep lanes", lanes) + shape, lambda: SP.make_batch(api, oracle, spec, lane_cases(oracle, spec, lanes)))
    assert len(b.hdr) == 8
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] >= 1).all(), G["info"]["iterations"]


def row_tie_case(O, spec):
    """two rows of one DPP row of 16 lanes with bit-equal slack: -y >= 0.05 on one control point of a segment and +y >= 0.05 on the next
    but one, where the free trajectory's y is exactly 0 -- both slacks are 0 - 0.05f in every form.  The lower id is the first candidate;
    its step takes the other's control point further down, so that one is a candidate behind it"""
    M, dim = spec["M"], spec["dim"]
    j1 = next(j for j in (6 * M * o + 6 * (M // 2) + 3 for o in range(_cap(M))) if (j % T) % 16 <= 13 and (j % T) // 64 == ((j + 2) % T) // 64)
    c = row_case(O, spec, [(j1, [0.0, -1.0, 0.0], 0.05), (j1 + 2, [0.0, 1.0, 0.0], 0.05)], seed=77, name="tie_inside_one_row_of_16_lanes")
    L = c.lsc.reshape(-1)
    assert L["d"][j1] == L["d"][j1 + 2] == np.float32(0.05) and np.array_equal(L["nrm"][j1], -L["nrm"][j1 + 2])
    assert np.abs(DC._free(O, spec, **_cut_agent(spec))[1]).max() < 1e-9
    assert (j1 % T) // 16 == ((j1 + 2) % T) // 16
    g, tr = RT._traced(O, c)
    cand = RT._candidates(tr)
    assert g["status"] == "optimal" and cand[0] == j1 and j1 + 2 in cand[1:], (j1, cand)
    return c


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_tie_between_two_wavefronts_and_inside_one_row_of_16_lanes_goes_to_the_lowest_id(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("ep ties",) + shape, lambda: SP.make_batch(api, oracle, spec, RT.twin_cases(oracle, spec) + [row_tie_case(oracle, spec)]))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] >= 1).all() and G["info"]["iterations"][2] >= 2, G["info"]["iterations"]


# ---- finish: the largest entry of the gradient scale in lane 0 and in lane 38 --------------------------------------------------------------
KQ = np.array([[720, -1800, 1200, 0, 0, -120], [-1800, 4800, -3600, 0, 600, 0], [1200, -3600, 3600, -1200, 0, 0],
               [0, 0, -1200, 3600, -3600, 1200], [0, 600, 0, -3600, 4800, -1800], [-120, 0, 0, 1200, -1800, 720]], float)


def fixed_part_entries(M, dim, ts, v0, a0, gk, q2s=1.0, wt2=2.0 * DC.W_T):
    """|c0| of finish_local's lanes (csrc/lscqp_das_body.inc): the reduced gradient at the plan's fixed part, lane = axis * NZA + a, the
    end-stop form (NZA = 3 (M - 1) + 1).  At a quiet instance's optimum the other operand of the lane's maximum, the reduced gradient
    itself, is rounding: these entries are the gradient scale's."""
    NZA = 3 * (M - 1) + 1
    out = np.zeros(dim * NZA)
    for zi in range(dim * NZA):
        kx, a = zi // NZA, zi % NZA
        last = a == 3 * (M - 1)
        m, j = (M - 1, 0) if last else (a // 3, a % 3)
        c1 = v0[kx] * DC.DT * 0.2
        c2 = a0[kx] * DC.DT * DC.DT * 0.05 + 2.0 * c1

        def g0(mm):
            g = np.array([q2s * (KQ[i, 1] * c1 + KQ[i, 2] * c2) if mm == 0 else 0.0 for i in range(6)])
            if mm >= M - ts:
                g[5] += -wt2 * gk[kx]
            return g

        g = g0(m)
        c0 = g[3] + g[4] + g[5] if last else g[3 + j]
        if m + 1 < M:
            w = [(0.0, 0.0, 1.0), (0.0, -1.0, -4.0), (1.0, 2.0, 4.0)][j]
            c0 += w[0] * g0(m + 1)[0] + w[1] * g0(m + 1)[1] + w[2] * g0(m + 1)[2]
        out[zi] = abs(c0)
    return out


def test_the_largest_entry_of_the_gradient_scale_in_lane_0_and_in_lane_38(api, oracle, torch_cuda):
    """M5 in 3-D, 39 lanes.  Lane 0 (axis 0, segment 0, first row): an agent already at its goal, moving along x -- the only entries are
    segment 0's, 2 400 c1 in lane 0 against 600 c1 in lane 1.  Lane 38 (axis 2, the end stop's row): an agent at rest with its goal
    along z and ONE terminal segment -- the entry is 2 w_t (goal - p0) there, 0.2 w_t in axis 0's such lane (the hop's 0.1 m aside)
    and 0 elsewhere.  The record's res_dual is the stationarity residual over max(1, that scale): the same bytes from every form."""
    M, dim = 5, 3
    spec = DC.spec_of(M, dim, "lsc")
    oc = DC.oracle_class(oracle, spec)
    p0 = DC._p0(spec)
    at_goal = dict(p0=p0, v0=np.array([0.3, 0.0, 0.0]), a0=np.zeros(3), goal=p0.copy(), next_waypoint=p0.copy(), nominal_velocity=1.0, radius=0.15)
    slow = float(np.hypot(1.0, 0.1)) / ((M + 2) * DC.DT)
    rest = DC._hop(spec, 2, 1.0, v=0.0, vn=slow)
    cases = [DC.Case("scale_in_lane_0", spec, oracle.make_agent(**dict(DC.LOOSE, **at_goal))), DC.Case("scale_in_lane_38", spec, oracle.make_agent(**dict(DC.LOOSE, **rest)))]
    ts = [oracle.terminal_segments(oc, c.agent) for c in cases]
    assert ts == [M, 1], ts
    e0 = fixed_part_entries(M, dim, ts[0], at_goal["v0"], at_goal["a0"], at_goal["goal"] - p0)
    e1 = fixed_part_entries(M, dim, ts[1], rest["v0"], rest["a0"], rest["goal"] - p0)
    assert len(e0) == 39 and int(np.argmax(e0)) == 0 and e0[0] > 2.0 * np.sort(e0)[-2] > 0.0, e0
    assert int(np.argmax(e1)) == 38 and e1[38] == 2.0 * DC.W_T and e1[38] > 2.0 * np.sort(e1)[-2] and e1[38] > 1.0, e1
    for c in cases:
        g = SP.restated(oracle, c)
        assert g["status"] == "optimal" and g["steps"] == 0, (c, g["status"], g["steps"])
    b = SP.batch(("ep scale",), lambda: SP.make_batch(api, oracle, spec, cases))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] == 0).all() and (G["info"]["res_dual"] <= 1e-9).all()
