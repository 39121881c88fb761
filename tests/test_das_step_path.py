"""The path of an instance that takes active-set steps (csrc/lscqp_das_body.inc behind its first pass): the later passes over the staged rows
with their clamped, untested loads, the factor and the class's table set up ahead of the first step, a joining row's descriptors stored
from registers, and behind them the steps, the leaving rows, the verification with multipliers and the proof of infeasibility -- on the
inputs at which an index, a tail slot, a position in the list of active rows or a budget of that code can go wrong.

Small batches (at most 8 instances) of the two smallest fused shapes, M5 in 3-D and M10 in 2-D, each through four forms of the kernel: the
fused launch (one test asserts that this form IS one launch), the two launches with 256 threads per instance, and the one- and
two-wavefront forms.  The fused forms of both shapes run the phase's latency text (LSCQP_DAS_FORM in csrc/lscqp_fused.hip), which holds the
rewritten step path; every other form here runs the throughput text, the step path as it was.  So "the same bytes in every form" compares
the latency text with the throughput text, and both with the oracle and the restatement.  Every instance expected OPTIMAL is finished by the phase, in the step count of the CPU restatement
(tests/das_reference.py) wherever that one decided every step by more than 1e-6 m, and held to the polished CPU oracle at the bars of
tests/test_das_families_gpu.py (x 1e-8 m, objective 1e-8 relative).  The builders assert their premises on the CPU: the oracle calls the
instance OPTIMAL, the restatement takes the intended steps, holds the intended rows and drops a row from the intended position."""
import numpy as np
import pytest

from tests import das_cases as DC
from tests import helpers as H
from tests.test_das_prologue import FORMS, SHAPE_IDS, SHAPES, Batch, _device_call, _kernel_launches, _relayout, _same, capacity_of

pytestmark = pytest.mark.gpu

X_TOL, OBJ_TOL = 1e-8, 1e-8  # tests/test_das_families_gpu.py
IP_X_TOL = 1e-6  # an instance the phase hands over is the interior-point pass's: its parity bar (smoke(), tests/test_gpu_parity.py)
OPTIMAL, INFEASIBLE, HANDED = "optimal", "proven infeasible", "handed over"
FAMILY_STEPS = {5: [1, 2, 1, 1], 10: [1, 3, 3, 1]}  # interval, velocity, acceleration, pair: steps of the case picked for the family
OBSTACLES = {5: [0, 1, 8, 9, 17, 18, 20], 10: [4, 5, 8, 9, 10]}  # LSC rows on both sides of 256 and 512 and at the instance's capacity


# ---- instances (DC.Case: spec, agent, lsc, sfc), premises asserted with the restatement -------------------------------------------------
def _lsc_agent(spec):
    p0 = DC._p0(spec)
    goal = p0 + np.array([1.0, 0.1, 0.0])
    return dict(p0=p0, v0=np.array([0.2, 0.0, 0.0]), a0=np.zeros(3), goal=goal, next_waypoint=goal.copy(), nominal_velocity=1.0, radius=0.15)


def plane_case(O, spec, n_obs, planes, seed, name):
    """DC.lsc_cases' agent among n_obs obstacles: `planes` cut its free trajectory, every other record is a plane with a random normal that
    stays a metre clear of it (a live row in every slot of the pass, never a candidate)"""
    M, dim = spec["M"], spec["dim"]
    a = _lsc_agent(spec)
    L = DC._plane_rows(O, spec, a, planes, n_obs)
    c = DC._free(O, spec, **a) + np.asarray(a["p0"], float)[:dim, None, None]
    rng = np.random.RandomState(seed)
    taken = {(oi, m) for (oi, m, _, _) in planes}
    for oi in range(n_obs):
        for m in range(M):
            if (oi, m) in taken:
                continue
            n = rng.randn(3)
            n[2] = n[2] if dim == 3 else 0.0
            n /= np.linalg.norm(n)
            vals = np.einsum("k,ki->i", n[:dim], c[:, m])
            at0 = float(n[:dim] @ np.asarray(a["p0"], float)[:dim])
            L["nrm"][oi, m] = n
            L["d"][oi, m] = float(np.float32(min(vals.min(), at0) - 1.0))
    return DC.Case(name, spec, O.make_agent(n_obs=n_obs, **dict(DC.LOOSE, **a)), lsc=L)


def leaving_recipe(O, spec, v, dist, fv, fc):
    """DC.leaving_cases' construction at one point of a wider grid: a hop under a velocity limit at fv of the free peak and a corridor face
    at fc of the free displacement mid-way"""
    M = spec["M"]
    a = DC._hop(spec, 0, 1.0, v=v, dist=dist)
    a["next_waypoint"] = a["p0"] + DC._unit(0, 0.5)
    c = DC._free(O, spec, **a)[0]
    cf = c.reshape(-1)
    vel = max(abs(cf[6 * m + i + 1] - cf[6 * m + i]) for m in range(M) for i in range(5) if not (m == 0 and i < 2)) / (DC.DT * 0.2)
    box = DC.wide_box(O, spec)
    box["bmax"][M // 2][0] = a["p0"][0] + fc * np.abs(c[M // 2]).max()
    return DC.Case("leaving_v%g_d%g_vel%g_face%g" % (v, dist, fv, fc), spec, O.make_agent(**dict(dict(vmax=[fv * vel, 30.0, 30.0], amax=[400.0] * 3), **a)), sfc=box)


_G = {}


def restated(O, c):
    if id(c) not in _G:
        _G[id(c)] = (c, DC.restate(O, c))
    return _G[id(c)][1]


def _designed(O, M, dim):
    return [c for c in DC.cases(O, M, dim, "lsc") if c.key == (M, dim, "lsc")]


def _pick(O, cases, what, ok):
    """the first designed case the restatement finishes with `ok`, those that decide every step clearly first"""
    found = [c for c in cases if restated(O, c)["status"] == "optimal" and ok(c, restated(O, c))]
    assert found, what
    return min(found, key=lambda c: (restated(O, c)["margin"] <= 1e-6, restated(O, c)["steps"]))


def quiet_case(O, spec):
    c = DC.Case("quiet", spec, O.make_agent(**dict(DC.LOOSE, **DC._hop(spec, 1, -1.0))))
    g = restated(O, c)
    assert g["status"] == "optimal" and g["steps"] == 0, g
    return c


def tail_cases(O, spec, cap):
    """one step on one LSC plane with n_obs * 6 M staged rows for every obstacle count of OBSTACLES -- the plane in the first or the last
    obstacle's slot by turns, on a middle segment -- and, without obstacles, one step on a corridor face"""
    M, dim = spec["M"], spec["dim"]
    assert max(OBSTACLES[M]) == cap, (OBSTACLES[M], cap)
    nL = [k * 6 * M for k in OBSTACLES[M]]
    assert all(any(a <= edge < b for a, b in zip(nL, nL[1:])) for edge in (256, 512)), nL
    out = []
    for i, k in enumerate(OBSTACLES[M]):
        if k == 0:
            c = _pick(O, _designed(O, M, dim), "one step on a two-sided row", lambda c, g: c.lsc is None and g["steps"] == 1)
        else:
            slot = 0 if i % 2 else k - 1
            c = plane_case(O, spec, k, [(slot, M // 2, [-0.75, 0.5, 0.25 if dim == 3 else 0.0], 0.6)], seed=100 + k, name="plane_of_%d" % k)
            g = restated(O, c)
            assert g["status"] == "optimal" and g["steps"] == 1 and g["active"][0][0] < k * 6 * M, (c, g["steps"], g["active"])
        out.append(c)
    return out


def family_and_held_cases(O, spec):
    """one step on an interval, a velocity, an acceleration and a pair row (fewest steps where the family needs more than one); then 2, 3
    and more than 8 rows held at the optimum"""
    M, dim = spec["M"], spec["dim"]
    D = _designed(O, M, dim)
    out = []
    for fam in ("interval", "velocity", "acceleration", "pair"):
        c = _pick(O, D, fam, lambda c, g: c.lsc is None and c.expect and c.expect.get("family") == fam and len(g["active"]) >= 1)
        out.append(c)
    # interval and pair rows in ONE step at both shapes; the velocity and acceleration limits of the designed cases (0.9 of the free peak)
    # bind on neighbouring stencils too, and their fewest are the counts below: a change to the case set that moves them is noticed here
    assert [restated(O, c)["steps"] for c in out] == FAMILY_STEPS[M], [(c.name, restated(O, c)["steps"]) for c in out]
    many = _pick(O, D, "more than 8 rows held", lambda c, g: len(g["active"]) > 8)
    return out + [held_case(O, spec, 2), held_case(O, spec, 3), many]


def held_case(O, spec, want):
    """a diagonal hop with `want` corridor faces across its way, each at 0.6 of the free displacement of its axis in its segment: the first
    choice of (axis, segment)s at which the restatement takes `want` steps, holds `want` rows and drops none"""
    import itertools

    M, dim = spec["M"], spec["dim"]
    p0 = DC._p0(spec)
    d = np.array([1.0, 1.0, 1.0 if dim == 3 else 0.0])
    a = dict(p0=p0, v0=0.2 * d, a0=np.zeros(3), goal=p0 + d, next_waypoint=p0 + d, nominal_velocity=1.0, radius=0.15)
    c = DC._free(O, spec, **a)
    for combo in itertools.combinations([(k, m) for m in (M // 2, 1, M - 1) for k in range(dim)], want):
        box = DC.wide_box(O, spec)
        for (k, m) in combo:
            box["bmax"][m][k] = p0[k] + 0.6 * np.abs(c[k][m]).max()
        case = DC.Case("faces_%s" % "_".join("k%dm%d" % km for km in combo), spec, O.make_agent(**dict(DC.LOOSE, **a)), sfc=box)
        g = restated(O, case)
        if g["status"] == "optimal" and g["steps"] == want and len(g["active"]) == want and not g["left"] and g["margin"] > 1e-6:
            return case
    raise AssertionError("no choice of %d faces holds %d rows in %d steps" % (want, want, want))


def leaving_cases(O, spec):
    """a row that leaves the list of active rows from its first, a middle and its last position"""
    M, dim = spec["M"], spec["dim"]
    D = _designed(O, M, dim)
    if M == 5:  # (no designed case of this shape drops a middle row; this point of the wider grid does)
        D = D + [leaving_recipe(O, spec, 0.8, 3.0, 0.3, 0.6)]
    where = dict(first=lambda l, kk: kk >= 2 and l == 0, middle=lambda l, kk: 0 < l < kk - 1, last=lambda l, kk: kk >= 2 and l == kk - 1)
    return [_pick(O, D, "a row leaves from the %s position" % pos, lambda c, g, f=f: any(f(l, kk) for (l, kk) in g["left"])) for pos, f in where.items()]


def infeasible_case(O, spec):
    """a plane across the way on one segment, and on that segment's last control point a second one with the opposite normal, 5 cm the wrong
    side of the first: rows of the first join, the second then finds no step and no multiplier to give way -- the proof inside the phase,
    with rows held (it reads the candidate's descriptors behind the loop of steps)"""
    from tests import das_reference as DR

    M = spec["M"]
    c = plane_case(O, spec, 3, [(0, M // 2, [-1.0, 0.0, 0.0], 0.6)], seed=9, name="opposite_planes")
    c.lsc["nrm"][2, M // 2, 5] = [1.0, 0.0, 0.0]
    c.lsc["d"][2, M // 2, 5] = np.float32(-c.lsc["d"][0, M // 2, 5] + np.float32(0.05))
    g = restated(O, c)
    assert g["status"] == DR.WHY_NO_STEP and g["steps"] >= 2 and len(g["active"]) >= 1 and g["margin"] > 1e-6, (g["status"], g["steps"], g["active"], g["margin"])
    assert DC.solve_oracle(O, c)["status"] != 0
    return c


def make_batch(api, O, spec, cases, expect=None, seed=5):
    oc = DC.oracle_class(O, spec)
    M = spec["M"]
    agents, lscs = [c.agent for c in cases], [c.lsc for c in cases]
    boxes = [c.sfc if c.sfc is not None else DC.wide_box(O, spec) for c in cases]
    hdr, rows, off, sfc = H.abi_batch(api, O, oc, agents, lscs, boxes, M)
    n_obs_max = int(hdr["n_obs"].max())
    if n_obs_max == 0:
        rows = off = None
    else:
        rows, off = _relayout(api, hdr, rows, off, M, seed=seed)  # (uneven offsets, NaN rows between the instances')
    b = Batch(DC.abi_desc(api, spec), oc, M, hdr, rows, off, sfc, n_obs_max, expect or [OPTIMAL] * len(cases), agents, lscs, boxes)
    b.cases = cases
    return b


_BATCHES = {}


def batch(key, make):
    if key not in _BATCHES:
        _BATCHES[key] = make()
    return _BATCHES[key]


# ---- the batch through every form ------------------------------------------------------------------------------------------------------
def every_form(api, O, torch, b, knobs=None):
    """the same bytes from every form; every instance what the batch expects of it"""
    res = [(name, _device_call(api, torch, b, dict(k, **(knobs or {})))) for name, k in FORMS]
    G = res[0][1]
    for name, r in res[1:]:
        assert _same(r, G), (name, r["status"], G["status"], r["info"], G["info"])
    if b.ref is None:
        b.ref = {}
        for q, e in enumerate(b.expect):
            if e != INFEASIBLE:
                r = O.solve(b.ocls, b.agents[q], b.lscs[q], b.boxes[q])
                assert r["status"] == 0, ("the oracle solves every feasible instance", q, b.cases[q])
                b.ref[q] = (r["x"], DC.objective(O.assemble(b.ocls, b.agents[q], b.lscs[q], b.boxes[q]), r["x"]))
    info = G["info"]
    for q, e in enumerate(b.expect):
        by_phase = bool(info["flags"][q] & api.INFO_ACTIVE_SET)
        if e == INFEASIBLE:
            print("step path| instance %d %s: status %d after %d steps, violation %.3g m" % (q, b.cases[q].name, G["status"][q], info["iterations"][q], info["res_primal"][q]))
            assert G["status"][q] == api.STATUS_INFEASIBLE and by_phase and info["iterations"][q] >= 2, (q, G["status"][q], info[q])
            continue
        xr, fr = b.ref[q]
        dx, dobj = np.abs(G["x"][q] - xr).max(), abs(G["obj"][q] - fr) / max(1.0, abs(fr))
        g = restated(O, b.cases[q])
        print("step path| instance %d %s: %s, %d steps (restatement %d, margin %.1e m), |dx| %.1e m, objective %.1e rel"
              % (q, b.cases[q].name, "by the phase" if by_phase else "handed over", info["iterations"][q], g["steps"], g["margin"], dx, dobj))
        assert G["status"][q] == api.STATUS_OPTIMAL, (q, G["status"][q], info[q])
        if e == OPTIMAL:
            assert by_phase, (q, info[q])
            assert dx <= X_TOL and dobj <= OBJ_TOL, (q, dx, dobj)
            if g["margin"] > 1e-6:
                assert info["iterations"][q] == g["steps"], (q, b.cases[q], info["iterations"][q], g["steps"])
        else:  # the interior-point pass solved it: no mark of the phase on the record
            assert not by_phase, (q, info[q])
            assert dx <= IP_X_TOL, (q, dx)
    return G


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_one_step_at_every_tail_shape_of_the_later_pass(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = batch(("tails",) + shape, lambda: make_batch(api, oracle, spec, tail_cases(oracle, spec, capacity_of(api, M, dim))))
    assert sorted(b.hdr["n_obs"]) == OBSTACLES[M] and len(b.hdr) <= 8
    G = every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] == 1).all(), G["info"]["iterations"]
    assert np.isfinite(G["x"]).all() and np.isfinite(G["obj"]).all()  # (nothing between the instances' rows was read)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_fused_form_is_one_launch_and_the_others_more(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = batch(("tails",) + shape, lambda: make_batch(api, oracle, spec, tail_cases(oracle, spec, capacity_of(api, M, dim))))
    assert _kernel_launches(api, torch_cuda, b, FORMS[0][1]) == 1
    for name, knobs in FORMS[1:]:
        assert _kernel_launches(api, torch_cuda, b, knobs) > 1, name


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_step_on_each_two_sided_family_and_two_three_and_many_rows_held(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = batch(("families",) + shape, lambda: make_batch(api, oracle, spec, family_and_held_cases(oracle, spec)))
    G = every_form(api, oracle, torch_cuda, b)
    assert G["info"]["iterations"][4] >= 2 and G["info"]["iterations"][5] >= 3 and G["info"]["iterations"][6] > 8, G["info"]["iterations"]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_row_leaves_from_the_first_a_middle_and_the_last_position_and_a_proof_with_rows_held(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = batch(("leaving",) + shape, lambda: make_batch(api, oracle, spec, leaving_cases(oracle, spec) + [infeasible_case(oracle, spec)],
                                                     expect=[OPTIMAL] * 3 + [INFEASIBLE]))
    G = every_form(api, oracle, torch_cuda, b)
    q = 3  # the start comes back, as for every instance the phase does not solve
    assert G["obj"][q] == 0.0 and np.array_equal(G["x"][q].reshape(dim, -1), np.repeat(b.hdr["p0"][q][:dim, None], 6 * M, axis=1))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_row_budget_and_the_step_budget_hand_over_alike_in_every_form(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")

    def make():
        fam = family_and_held_cases(oracle, spec)
        return make_batch(api, oracle, spec, [fam[0], fam[4], fam[5]])  # one step and one row; two rows; three rows

    b = batch(("budgets",) + shape, make)
    g = [restated(oracle, c) for c in b.cases]
    assert g[0]["steps"] == 1 and g[1]["peak"] == 2 and g[2]["peak"] == 3 and g[1]["steps"] == 2 and g[2]["steps"] == 3, [(x["steps"], x["peak"]) for x in g]
    for knobs, expect in ((dict(das_kmax=2), [OPTIMAL, OPTIMAL, HANDED]), (dict(das_kmax=1), [OPTIMAL, HANDED, HANDED]),
                          (dict(das_steps=2), [OPTIMAL, OPTIMAL, HANDED]), (dict(das_steps=1), [OPTIMAL, HANDED, HANDED])):
        b.expect = expect
        every_form(api, oracle, torch_cuda, b, knobs=knobs)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_quiet_instance_beside_a_stepping_one_in_both_orders(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    cap = capacity_of(api, M, dim)
    step = batch(("stepper",) + shape, lambda: plane_case(oracle, spec, cap, [(cap - 1, M // 2, [-1.0, 0.0, 0.0], 0.6)], seed=3, name="stepper"))
    quiet = batch(("quiet",) + shape, lambda: quiet_case(oracle, spec))
    out = []
    for order in ((quiet, step), (step, quiet)):
        b = make_batch(api, oracle, spec, list(order))
        G = every_form(api, oracle, torch_cuda, b)
        out.append({c.name: (G["x"][q].tobytes(), G["obj"][q].tobytes(), int(G["info"]["iterations"][q])) for q, c in enumerate(order)})
    assert out[0] == out[1] and out[0]["quiet"][2] == 0 and out[0]["stepper"][2] == 1
