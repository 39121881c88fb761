"""Each thread's LSC rows kept in registers across the loop of steps and the first pass in one block of requests (csrc/lscqp_das_body.inc,
the latency text, LSCQP_DAS_FORM LSCQP_DAS_LATENCY) -- on the inputs at which a row slot, a dropped row, a slot past the instance's last row or the
pass's minimum over the wavefronts can go wrong.

Small batches (at most 8 instances) of the two fused shapes that run the latency text, M5 in 3-D and M10 in 2-D, each through the four forms of
tests/test_das_prologue.py: the fused launch (the new text; one test asserts that this form IS one launch), the two launches and the one-
and two-wavefront forms (the text as it was).  Every form must return the same bytes in x, obj, status and info -- new text against old;
every instance expected OPTIMAL is finished by the phase, in the step count of the CPU restatement (tests/das_reference.py) wherever that
one decided every step by more than 1e-6 m, and held to the polished CPU oracle at 1e-8 m / 1e-8 relative (tests/test_das_step_path.py:
every_form).  The builders assert their premises on the CPU with the restatement's trace: LSC row j = 6 M o + 6 m + i (obstacle o, segment
m, control point i) is thread j mod 256's, in that thread's slot j div 256; two-sided row r is thread r mod 256's."""
import numpy as np
import pytest

from tests import das_cases as DC
from tests import test_das_prologue as PR
from tests import test_das_round_trips as RT
from tests import test_das_step_path as SP
from tests.test_das_prologue import FORMS, SHAPE_IDS, SHAPES, _device_call, _kernel_launches, _same

pytestmark = pytest.mark.gpu

OPTIMAL, INFEASIBLE, HANDED = SP.OPTIMAL, SP.INFEASIBLE, SP.HANDED
T = RT.T
OBLIQUE = RT.OBLIQUE
FAMILIES = ("interval", "velocity", "acceleration", "pair")


def _traced(O, c):
    return RT._traced(O, c)


def _cap(M):
    return max(SP.OBSTACLES[M])


def _place(M, u, w):
    """(obstacle, segment) whose six rows all lie in slot u of wavefront w's threads: rows [256 u + 64 w, 256 u + 64 w + 64); None where the
    shape's 6 M cap rows do not reach that slot of that wavefront"""
    lo, hi = 256 * u + 64 * w, 256 * u + 64 * w + 64
    segs = sorted(range(1, M), key=lambda m: abs(m - M // 2))  # (the middle segment first; never segment 0: its first rows are dropped)
    for o in range(_cap(M)):
        for m in segs:
            if lo <= 6 * M * o + 6 * m and 6 * M * o + 6 * m + 5 < hi:
                return o, m
    return None


def _slot(row):
    return row // T


def _wave(row):
    return (row % T) >> 6


# ---- the candidate in each slot of each wavefront --------------------------------------------------------------------------------------
def slot_cases(O, spec, u):
    """a full instance (the cap's obstacles: every slot of every thread holds a live row or lies past the end) whose one cutting plane is a
    row of slot u in wavefront 0, 1, 2, 3 in turn"""
    M, dim = spec["M"], spec["dim"]
    out = []
    for w in range(4):
        at = _place(M, u, w)
        if at is None:
            continue
        o, m = at
        c = SP.plane_case(O, spec, _cap(M), [(o, m, OBLIQUE[dim], 0.6)], seed=70 + 4 * u + w, name="plane_in_slot_%d_of_wavefront_%d" % (u, w))
        g, tr = _traced(O, c)
        assert g["status"] == "optimal" and g["steps"] >= 1 and tr[0]["family"] == "lsc" and (_slot(tr[0]["row"]), _wave(tr[0]["row"])) == (u, w), (c, tr[:1])
        out.append(c)
    return out


@pytest.mark.parametrize("u", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_candidate_in_each_slot_of_each_wavefront_that_has_one(api, oracle, torch_cuda, shape, u):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rr slots", u) + shape, lambda: SP.make_batch(api, oracle, spec, slot_cases(oracle, spec, u)))
    nL = 6 * M * _cap(M)
    assert len(b.cases) == len([w for w in range(4) if 256 * u + 64 * w < nL]) >= 2  # (600 rows: slot 2 is wavefront 0's, 1's and part of 2's)
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] >= 1).all(), G["info"]["iterations"]


# ---- row counts on both sides of the slots' boundaries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_row_counts_on_both_sides_of_256_and_512_permuted_and_the_fused_form_is_one_launch(api, oracle, torch_cuda, shape):
    """n_obs = 0, 1, 8, 9, 17, 18, 20 at M5 in 3-D (240 | 270 and 510 | 540 rows; 20 is the cap), 4, 5, 8, 9, 10 at M10 in 2-D: one step
    each, the instances at uneven row offsets and taken in a permuted order"""
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    tails = SP.batch(("tails",) + shape, lambda: SP.make_batch(api, oracle, spec, SP.tail_cases(oracle, spec, PR.capacity_of(api, M, dim))))
    assert sorted(tails.hdr["n_obs"]) == SP.OBSTACLES[M] and tails.off is not None  # (SP.make_batch: uneven offsets, NaN between the instances)
    plain = SP.every_form(api, oracle, torch_cuda, tails)
    n = len(tails.hdr)
    perm = [(3 * q + 2) % n for q in range(n)]
    assert sorted(perm) == list(range(n)) and perm != list(range(n))
    tails.order = perm
    try:
        res = [_device_call(api, torch_cuda, tails, knobs) for _, knobs in FORMS]
    finally:
        tails.order = None
    assert all(_same(r, plain) for r in res)  # (an instance's result does not depend on which workgroup took it)
    assert (plain["info"]["iterations"] == 1).all()
    assert _kernel_launches(api, torch_cuda, tails, FORMS[0][1]) == 1


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_launch_of_one_full_instance(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rr one",) + shape, lambda: SP.make_batch(api, oracle, spec, slot_cases(oracle, spec, 2)[:1]))
    assert len(b.hdr) == 1 and int(b.hdr["n_obs"][0]) == _cap(M)
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert G["info"]["iterations"][0] >= 1


# ---- candidates in different slots in turn; the row budget behind live registers ----------------------------------------------------------
def turns_case(O, spec):
    """a diagonal hop across three planes in three segments, rows of slot 0, 1 and 2: three or more steps whose LSC candidates lie in all
    three slots (the first choice of fractions and segments at which the restatement finds them so, every step decided clearly)"""
    import itertools

    M, dim = spec["M"], spec["dim"]
    p0 = DC._p0(spec)
    d = np.array([1.0, 1.0, 1.0 if dim == 3 else 0.0])
    a = dict(p0=p0, v0=0.2 * d, a0=np.zeros(3), goal=p0 + d, next_waypoint=p0 + d, nominal_velocity=1.0, radius=0.15)
    obs = [next(o for o in range(_cap(M)) if _slot(6 * M * o) == u and _slot(6 * M * o + 6 * M - 1) == u) for u in (0, 1, 2)]
    # one plane across each axis' way (the objective couples no two axes: each of them binds); in 2-D the third across the diagonal
    nrm = [[-1.0, 0.25, 0.0], [0.25, -1.0, 0.0], [0.0, 0.25, -1.0] if dim == 3 else [-1.0, -1.0, 0.0]]
    for fr, segs in itertools.product(((0.5, 0.5, 0.5), (0.3, 0.5, 0.5), (0.5, 0.3, 0.6), (0.3, 0.5, 0.8)), itertools.permutations((1, M // 2, M - 1))):
        planes = [(obs[i], segs[i], nrm[i], fr[i]) for i in range(3)]
        L = DC._plane_rows(O, spec, a, planes, _cap(M))
        case = DC.Case("turns_%s_%s" % ("_".join(map(str, segs)), "_".join(map(str, fr))), spec, O.make_agent(n_obs=_cap(M), **dict(DC.LOOSE, **a)), lsc=L)
        g, tr = _traced(O, case)
        cand = RT._candidates(tr)
        if g["status"] == "optimal" and g["margin"] > 1e-6 and g["peak"] <= 10 and {_slot(r) for r in cand if r < L.size} == {0, 1, 2}:
            assert g["steps"] >= 3
            return case
    raise AssertionError("no choice takes candidates from all three slots")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_candidates_in_different_slots_in_turn_and_the_row_budget_behind_them(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rr turns",) + shape, lambda: SP.make_batch(api, oracle, spec, [turns_case(oracle, spec), SP.quiet_case(oracle, spec)]))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert G["info"]["iterations"][0] >= 3 and G["info"]["iterations"][1] == 0
    # one active row allowed: the second candidate ends the phase, and the interior-point pass runs in the same workgroup behind it
    b.expect = [HANDED, OPTIMAL]
    try:
        SP.every_form(api, oracle, torch_cuda, b, knobs=dict(das_kmax=1))
    finally:
        b.expect = [OPTIMAL, OPTIMAL]


# ---- rows that translate drops -------------------------------------------------------------------------------------------------------------
def dropped_case(O, spec):
    """a plane to step on, and beside it in every slot a row that would be the most violated one if it counted: a zero normal with a
    positive bound (0 >= 5 never holds), and a deep cut on each of the first three control points of segment 0"""
    M, dim = spec["M"], spec["dim"]
    o_step, m_step = _place(M, 1, 1)
    c = SP.plane_case(O, spec, _cap(M), [(o_step, m_step, OBLIQUE[dim], 0.6)], seed=91, name="dropped_rows")
    L = c.lsc
    for u in (0, 1, 2):
        o, m = _place(M, u, 0)
        assert (o, m) != (o_step, m_step)
        L["nrm"][o, m, 4] = 0.0
        L["d"][o, m, 4] = np.float32(5.0)
    o0 = _place(M, 2, 1)[0]  # (segment 0 of an obstacle of the last slot)
    for i in range(3):
        L["nrm"][o0, 0, i] = [-1.0, 0.0, 0.0]
        L["d"][o0, 0, i] = np.float32(3.0)  # -x >= 3 at x = 0
    g, tr = _traced(O, c)
    assert g["status"] == "optimal" and g["steps"] >= 1 and all(_slot(s["row"]) == 1 for s in tr), (g["status"], tr)
    return c


def zero_only_case(O, spec):
    """no row to step on: the dropped rows alone -- a quiet instance whose every wavefront holds a would-be violated row"""
    M, dim = spec["M"], spec["dim"]
    c = SP.plane_case(O, spec, _cap(M), [], seed=92, name="dropped_rows_only")
    for w in range(4):
        o, m = _place(M, w % 2, w)
        c.lsc["nrm"][o, m, 3] = 0.0
        c.lsc["d"][o, m, 3] = np.float32(5.0)
    g = SP.restated(O, c)
    assert g["status"] == "optimal" and g["steps"] == 0, g
    return c


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_rows_that_translate_drops_are_no_candidates_in_any_pass(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rr dropped",) + shape, lambda: SP.make_batch(api, oracle, spec, [dropped_case(oracle, spec), zero_only_case(oracle, spec)]))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert G["info"]["iterations"][0] >= 1 and G["info"]["iterations"][1] == 0


# ---- a row that leaves and rejoins; the proof of infeasibility ---------------------------------------------------------------------------------
def _rejoins(tr):
    """a row that is a candidate again after it has left the list of active rows"""
    held, gone = [], set()
    for s in tr:
        if s["row"] in gone:
            return True
        if s["leaves"] >= 0:
            gone.add(held.pop(s["leaves"]))
        elif np.isfinite(s["t2"]):
            held.append(s["row"])
    return False


# four planes across the way of SP._lsc_agent at M5 in 3-D (obstacle, segment, normal, fraction: found by a seeded search over such sets):
# row 417 joins first, leaves on the second candidate's first partial step and is the candidate again four steps later
REJOIN_M5 = [(13, 4, [-0.7822351455688477, -0.025503434240818024, 0.6224610209465027], 0.22),
             (18, 2, [-0.7732364535331726, 0.6108874082565308, -0.17006458342075348], 0.62),
             (10, 4, [-0.7348635792732239, 0.6359297037124634, -0.2357306182384491], 0.84),
             (13, 1, [-0.8530397415161133, 0.4310290813446045, 0.2941720187664032], 0.25)]


def rejoining_case(O, spec):
    """M5 in 3-D: an LSC row (a thread's second slot) that leaves and rejoins, every step decided clearly; M10 in 2-D: the designed case in
    which a two-sided row does (no LSC rows; its closest decision is below 1e-6 m, so its step count is not held to the restatement's)"""
    M, dim = spec["M"], spec["dim"]
    if (M, dim) == (5, 3):
        a = SP._lsc_agent(spec)
        c = DC.Case("lsc_row_leaves_and_rejoins", spec, O.make_agent(n_obs=_cap(M), **dict(DC.LOOSE, **a)), lsc=DC._plane_rows(O, spec, a, REJOIN_M5, _cap(M)))
        g, tr = _traced(O, c)
        assert g["status"] == "optimal" and g["margin"] > 1e-6 and g["left"] and _rejoins(tr) and all(s["row"] < c.lsc.size for s in tr), (g["status"], g["margin"], tr)
        return c
    return SP._pick(O, SP._designed(O, M, dim), "a row that leaves and rejoins", lambda c, g: bool(g["left"]) and _rejoins(_traced(O, c)[1]))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_row_that_leaves_and_rejoins_and_a_proof_of_infeasibility_with_rows_held(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rr rejoin",) + shape, lambda: SP.make_batch(api, oracle, spec, [rejoining_case(oracle, spec), SP.infeasible_case(oracle, spec)],
                                                             expect=[OPTIMAL, INFEASIBLE]))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert G["info"]["iterations"][0] >= 3  # (joins, leaves, joins again)


# ---- a NaN in a live row of each wavefront --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_nan_in_a_live_row_of_each_wavefront_is_numeric_in_every_form(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")

    def make():
        cases = [SP.plane_case(oracle, spec, _cap(M), [], seed=80 + w, name="clear_but_for_a_nan_in_wavefront_%d" % w) for w in range(4)]
        b = SP.make_batch(api, oracle, spec, cases + [SP.quiet_case(oracle, spec)])
        b.rows = b.rows.copy()
        for w in range(4):
            o, m = _place(M, (2, 1, 0, 1)[w], w)  # (the thread's third, second, first and second slot)
            j = int(b.off[w]) + 6 * M * o + 6 * m + 4
            assert np.isfinite(b.rows["b"][j]) and b.rows["nx"][j] != 0.0
            b.rows["nx" if w % 2 else "b"][j] = np.nan
        return b

    b = SP.batch(("rr nan",) + shape, make)
    for c in b.cases[:4]:
        assert SP.restated(oracle, c)["steps"] == 0  # (without the NaN every wavefront of these instances is quiet)
    res = [(name, _device_call(api, torch_cuda, b, knobs)) for name, knobs in FORMS]
    for name, r in res[1:]:
        assert _same(r, res[0][1]), (name, r["status"], res[0][1]["status"])
    G = res[0][1]
    assert list(G["status"]) == [api.STATUS_NUMERIC] * 4 + [api.STATUS_OPTIMAL], G["status"]


# ---- two-sided candidates of each family on each side ------------------------------------------------------------------------------------------
def family_side_cases(O, spec):
    """per family and side the designed case with the fewest steps that has such a candidate; a (family, side) no designed case of the
    shape steps on is named in the assertion"""
    M, dim = spec["M"], spec["dim"]
    D = [c for c in SP._designed(O, M, dim) if c.lsc is None]
    out, missing = [], []
    for fam in FAMILIES:
        for side in (0, 1):
            found = [c for c in D if SP.restated(O, c)["status"] == "optimal" and any(s["family"] == fam and (s["row"] & 1) == side for s in _traced(O, c)[1])]
            if not found:
                missing.append((fam, side))
                continue
            c = min(found, key=lambda c: (SP.restated(O, c)["margin"] <= 1e-6, SP.restated(O, c)["steps"]))
            if not any(c is x for x in out):
                out.append(c)
    assert not missing, missing
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_two_sided_candidates_of_each_family_on_each_side(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rr sides",) + shape, lambda: SP.make_batch(api, oracle, spec, family_side_cases(oracle, spec)))
    assert len(b.hdr) <= 8
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] >= 1).all()


def test_a_candidate_in_a_threads_second_two_sided_slot_beside_full_lsc_slots(api, oracle, torch_cuda):
    """M10 in 2-D (390 two-sided rows: two slots a thread): the candidate is a two-sided row r >= 256, once without LSC rows and once
    in the batch of a full instance, whose registers hold three live LSC rows a thread"""
    M, dim = 10, 2
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rr second",) + (M, dim), lambda: SP.make_batch(api, oracle, spec, [RT.second_slot_case(oracle, M, dim)] + slot_cases(oracle, spec, 2)[:1]))
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] >= 1).all()
