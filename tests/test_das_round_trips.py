"""The one-read LDS waits folded in the fused phase (csrc/lscqp_das_body.inc, the latency text): the empty-interval verdict
from one read of the four ballots, the pass's cross-wavefront minimum by selects, `primal` read with the step's decision, a two-sided
candidate's stencil and bounds in one request, the candidate's multiplier kept in a register beside ctl_[3], and each thread's two-sided
rows kept in registers across the loop of steps -- on the inputs at which a slot, a tie, a side or a sum of that code can go wrong.

Small batches (at most 8 instances) of the two fused shapes that run the latency text, M5 in 3-D and M10 in 2-D, each through the four forms of
tests/test_das_prologue.py: the fused launch (the new text; one test asserts that this form IS one launch), the two launches and the one-
and two-wavefront forms (the text as it was).  Every form must return the same bytes in x, obj, status and info -- new text against old;
every instance expected OPTIMAL is finished by the phase, in the step count of the CPU restatement (tests/das_reference.py) wherever that
one decided every step by more than 1e-6 m, and held to the polished CPU oracle at 1e-8 m / 1e-8 relative (tests/test_das_step_path.py:
every_form).  The builders assert their premises on the CPU with the restatement's trace: which row is the candidate of which step, in
which wavefront's slot it lies (LSC row j and two-sided row r are thread j mod 256's and r mod 256's), which row leaves, which partial
step moves no point."""
import numpy as np
import pytest

from tests import das_cases as DC
from tests import test_das_prologue as PR
from tests import test_das_step_path as SP
from tests.test_das_prologue import FORMS, SHAPE_IDS, SHAPES, _device_call, _kernel_launches, _same

pytestmark = pytest.mark.gpu

OPTIMAL, EMPTY = SP.OPTIMAL, PR.EMPTY
T = 256  # threads of the fused phase
# (slot, ...) of the obstacle whose plane cuts the middle segment: its six rows lie in wavefront 0, 1, 2, 3 (row 6 M o + 6 (M // 2) + i)
WAVE_SLOTS = {5: [0, 2, 4, 6], 10: [0, 1, 2, 3]}
# two obstacles with the same plane: the lower ids in the lower wavefront; the lower ids (about 100: wavefront 1's first slot) in the
# HIGHER wavefront, the others (about 300: wavefront 0's second slot) in the lower one
TWIN_SLOTS = {5: [(0, 2), (3, 9)], 10: [(0, 1), (1, 4)]}
OBLIQUE = {3: [-0.75, 0.5, 0.25], 2: [-0.75, 0.5, 0.0]}


def _traced(O, c):
    """(restatement, trace) of one case, once"""
    if not hasattr(c, "_trace"):
        tr = []
        c._g, c._trace = DC.restate(O, c, trace=tr), tr
    return c._g, c._trace


def _n_lsc(c):
    return 0 if c.lsc is None else int(np.asarray(c.lsc).size)


def _wave_of(c, row):
    """the wavefront whose thread holds row `row` in the pass"""
    nL = _n_lsc(c)
    return ((row if row < nL else (row - nL) >> 1) % T) >> 6


def _candidates(tr):
    """the candidate rows in the order the passes found them (a candidate's partial steps are one entry)"""
    out = []
    for s in tr:
        if not out or out[-1] != s["row"]:
            out.append(s["row"])
    return out


# ---- a: the empty-interval verdict ----------------------------------------------------------------------------------------------------
def empty_batch(api, O, M, dim):
    """corridor boxes beyond the world box on a control point whose interval row (r = axis * 6 M + control point < 128) lies in
    wavefront 0 alone, in wavefront 1 alone, in both; and a feasible instance"""
    spec = DC.spec_of(M, dim, "lsc")
    oc = DC.oracle_class(O, spec)
    P = 6 * M
    k1 = dim - 1  # the last axis: its rows from control point 4 (3-D, r = 60 + cp) or 4 (2-D at M = 10, r = 60 + cp) on are wavefront 1's
    assert k1 * P + 6 >= 64 and k1 * P + 11 < 128 and P <= 64
    where = [[(0, M - 1)], [(k1, 1)], [(0, M - 1), (k1, 1)], []]
    agents = [O.make_agent(**dict(DC.LOOSE, **DC._hop(spec, q % dim, 1.0 if q % 2 else -1.0))) for q in range(len(where))]
    boxes = []
    for w in where:
        b = DC.wide_box(O, spec)
        for (k, m) in w:
            b["bmin"][m][k], b["bmax"][m][k] = spec["world_max"][k] + 1.0, spec["world_max"][k] + 2.0
        boxes.append(b)
    hdr, rows, off, sfc = SP.H.abi_batch(api, O, oc, agents, [None] * len(agents), boxes, M)
    expect = [EMPTY if w else OPTIMAL for w in where]
    return PR.Batch(DC.abi_desc(api, spec), oc, M, hdr, None, None, sfc, 0, expect, agents, [None] * len(agents), boxes)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_an_empty_interval_in_wavefront_0_in_wavefront_1_in_both_and_in_none(api, oracle, torch_cuda, shape):
    M, dim = shape
    b = PR.batch(("rt empty",) + shape, empty_batch, api, oracle, M, dim)
    G = PR.every_form(api, oracle, torch_cuda, b)
    assert list(G["status"]) == [api.STATUS_INFEASIBLE] * 3 + [api.STATUS_OPTIMAL]
    assert (G["info"]["res_primal"][:3] >= 1.0).all()  # the overlap lo - hi: the box lies a metre beyond the world's face


# ---- b: the pass's minimum across the wavefronts ----------------------------------------------------------------------------------------
def wave_cases(O, spec):
    """one cutting plane, in the obstacle slot whose rows lie in wavefront 0, 1, 2, 3 in turn"""
    M, dim = spec["M"], spec["dim"]
    out = []
    for w, slot in enumerate(WAVE_SLOTS[M]):
        c = SP.plane_case(O, spec, max(WAVE_SLOTS[M]) + 2, [(slot, M // 2, OBLIQUE[dim], 0.6)], seed=40 + w, name="plane_in_wavefront_%d" % w)
        g, tr = _traced(O, c)
        assert g["status"] == "optimal" and g["steps"] >= 1 and tr[0]["family"] == "lsc" and _wave_of(c, tr[0]["row"]) == w, (c, w, tr[:1])
        out.append(c)
    return out


def twin_cases(O, spec):
    """two obstacles with the same plane: rows with bit-equal slack in different wavefronts -- the lower id must win"""
    M, dim = spec["M"], spec["dim"]
    out = []
    for (a, b) in TWIN_SLOTS[M]:
        c = SP.plane_case(O, spec, b + 1, [(a, M // 2, OBLIQUE[dim], 0.6), (b, M // 2, OBLIQUE[dim], 0.6)], seed=50 + a, name="twins_%d_%d" % (a, b))
        L = np.asarray(c.lsc)
        assert np.array_equal(L["nrm"][a, M // 2], L["nrm"][b, M // 2]) and np.array_equal(L["d"][a, M // 2], L["d"][b, M // 2])
        g, tr = _traced(O, c)
        lo, hi = tr[0]["row"], tr[0]["row"] + (b - a) * 6 * M
        assert g["status"] == "optimal" and a * 6 * M <= lo < (a + 1) * 6 * M and _wave_of(c, lo) != _wave_of(c, hi), (c, tr[:1])
        out.append(c)
    assert _wave_of(out[0], _traced(O, out[0])[1][0]["row"]) == 0  # the lower id in the lower wavefront ...
    lo = _traced(O, out[1])[1][0]["row"]
    assert _wave_of(out[1], lo) == 1 and _wave_of(out[1], lo + (TWIN_SLOTS[M][1][1] - TWIN_SLOTS[M][1][0]) * 6 * M) == 0  # ... and in the higher one
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_minimum_in_each_wavefront_ties_across_wavefronts_and_a_two_sided_minimum(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")

    def make():
        two_sided = SP._pick(oracle, SP._designed(oracle, M, dim), "a step on a two-sided row", lambda c, g: c.lsc is None and g["steps"] == 1)
        return SP.make_batch(api, oracle, spec, wave_cases(oracle, spec) + twin_cases(oracle, spec) + [two_sided])

    b = SP.batch(("rt waves",) + shape, make)
    assert len(b.hdr) <= 8
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] >= 1).all(), G["info"]["iterations"]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_nan_in_one_row_is_numeric_in_every_form(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")

    def make():
        b = SP.make_batch(api, oracle, spec, [SP.quiet_case(oracle, spec)] + wave_cases(oracle, spec)[1:3])
        b.rows = b.rows.copy()
        j = int(b.off[2]) + WAVE_SLOTS[M][2] * 6 * M + 6 * (M // 2) + 4  # a live row of the third instance, in wavefront 2
        assert np.isfinite(b.rows["b"][j]) and b.rows["nx"][j] != 0.0
        b.rows["b"][j] = np.nan
        return b

    b = SP.batch(("rt nan",) + shape, make)
    res = [(name, _device_call(api, torch_cuda, b, knobs)) for name, knobs in FORMS]
    for name, r in res[1:]:
        assert _same(r, res[0][1]), (name, r["status"], res[0][1]["status"])
    G = res[0][1]
    assert list(G["status"]) == [api.STATUS_OPTIMAL, api.STATUS_OPTIMAL, api.STATUS_NUMERIC], G["status"]
    assert G["info"]["iterations"][0] == 0 and G["info"]["iterations"][1] >= 1 and np.isfinite(G["x"][:2]).all()


# ---- c, d, e: the step's decision, a two-sided candidate, the candidate's multiplier -------------------------------------------------------
def dependent_case(O, spec):
    """A corridor face on the last control point of the middle segment and an LSC row with HALF the face's normal on the same control
    point, a tenth of the free displacement stricter: the face is the more violated row (raw slack) and joins first; the LSC row is then the candidate and its normal
    lies in the span of the face's -- a partial step without a primal move, on which the face leaves, and a second one, taken with no row
    held, on which the candidate joins with the multiplier the first one left it."""
    M, dim = spec["M"], spec["dim"]
    a = DC._hop(spec, 0, 1.0, v=0.2)
    m = M // 2
    c = DC._free(O, spec, **a)[0]
    far = float(c[m, 5])
    assert far > 0.05 and far == c[m].max()
    hi, hi2 = a["p0"][0] + 0.6 * far, a["p0"][0] + 0.5 * far  # raw slacks at the free point: -0.4 far (the face), -0.25 far (the half normal)
    box = DC.wide_box(O, spec)
    box["bmax"][m][0] = hi
    L = np.zeros((1, M, 6), O.LSC_DTYPE)
    L["nrm"][0, m, 5] = [-0.5, 0.0, 0.0]
    L["d"][0, m, 5] = float(np.float32(-0.5 * hi2))
    return DC.Case("half_normal_on_a_face", spec, O.make_agent(n_obs=1, **dict(DC.LOOSE, **a)), lsc=L, sfc=box)


def decision_cases(O, spec):
    """candidates: a velocity row on its lower side, one on its upper side, an acceleration row, an LSC row; a candidate that needs two
    partial steps because a row leaves first; a partial step without a primal move"""
    M, dim = spec["M"], spec["dim"]
    D = SP._designed(O, M, dim)

    def has(c, fam, side=None):
        g, tr = _traced(O, c)
        return g["status"] == "optimal" and any(s["family"] == fam and (side is None or (s["row"] - _n_lsc(c)) & 1 == side) for s in tr)

    def pick(what, ok):
        found = [c for c in D if c.lsc is None and ok(c)]
        assert found, what
        return min(found, key=lambda c: (_traced(O, c)[0]["margin"] <= 1e-6, _traced(O, c)[0]["steps"]))

    out = [pick("a velocity row on its lower side", lambda c: has(c, "velocity", 0)), pick("a velocity row on its upper side", lambda c: has(c, "velocity", 1)),
           pick("an acceleration row", lambda c: has(c, "acceleration")),
           SP.plane_case(O, spec, 3, [(1, M // 2, OBLIQUE[dim], 0.6)], seed=60, name="lsc_candidate")]
    assert has(out[3], "lsc")
    leaving = SP.leaving_cases(O, spec)[0]
    g, tr = _traced(O, leaving)
    rows = [s["row"] for s in tr]
    assert any(s["leaves"] >= 0 for s in tr) and any(rows[i] == rows[i + 1] for i in range(len(rows) - 1)), tr  # two partial steps of one candidate
    dep = dependent_case(O, spec)
    g, tr = _traced(O, dep)
    still = [s for s in tr if not np.isfinite(s["t2"]) and np.isfinite(s["t1"])]
    assert g["status"] == "optimal" and still and still[0]["leaves"] >= 0 and still[0]["family"] == "lsc", (g["status"], tr)
    nxt = tr[tr.index(still[0]) + 1]
    assert nxt["row"] == still[0]["row"] and nxt["held"] == still[0]["held"] - 1, tr  # the same candidate again, one row fewer held
    return out + [leaving, dep]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_candidates_of_every_kind_a_leaving_row_and_a_partial_step_without_a_primal_move(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")
    b = SP.batch(("rt decisions",) + shape, lambda: SP.make_batch(api, oracle, spec, decision_cases(oracle, spec)))
    assert len(b.hdr) <= 8
    G = SP.every_form(api, oracle, torch_cuda, b)
    g = _traced(oracle, b.cases[-1])[0]
    assert G["info"]["iterations"][-1] == g["steps"] >= 3, (G["info"]["iterations"], g["steps"])  # (the face, the still step, the join)


# ---- f: the two-sided rows in registers across the loop of steps --------------------------------------------------------------------------
def alternating_case(O, spec):
    """a diagonal hop with a plane deep across one segment, a corridor face of the other axis across a second and a shallow plane across a
    third: three or more steps whose candidates come from the LSC rows, the two-sided rows and the LSC rows again (the first choice of
    fractions and segments at which the restatement finds them so, every step decided clearly)"""
    import itertools

    M, dim = spec["M"], spec["dim"]
    p0 = DC._p0(spec)
    d = np.array([1.0, 1.0, 1.0 if dim == 3 else 0.0])
    a = dict(p0=p0, v0=0.2 * d, a0=np.zeros(3), goal=p0 + d, next_waypoint=p0 + d, nominal_velocity=1.0, radius=0.15)
    c = DC._free(O, spec, **a)
    nrm = [-1.0, 0.25, 0.0]
    for fa, ff, fb, (ma, mf, mb) in itertools.product((0.3, 0.5), (0.65, 0.5), (0.9, 0.8), ((M - 1, M // 2, 1), (M - 1, 1, M // 2))):
        L = DC._plane_rows(O, spec, a, [(0, ma, nrm, fa), (1, mb, nrm, fb)], 2)
        box = DC.wide_box(O, spec)
        box["bmax"][mf][1] = p0[1] + ff * np.abs(c[1][mf]).max()
        case = DC.Case("planes_m%d_%.1f_m%d_%.1f_face_m%d_%.2f" % (ma, fa, mb, fb, mf, ff), spec, O.make_agent(n_obs=2, **dict(DC.LOOSE, **a)), lsc=L, sfc=box)
        g, tr = _traced(O, case)
        kinds = [r < _n_lsc(case) for r in _candidates(tr)]
        turns = sum(1 for i in range(len(kinds) - 1) if kinds[i] != kinds[i + 1])
        if g["status"] == "optimal" and g["steps"] >= 3 and turns >= 2 and g["margin"] > 1e-6 and g["peak"] <= 10:
            return case
    raise AssertionError("no choice alternates between LSC and two-sided candidates")


def second_slot_case(O, M, dim):
    """M10 in 2-D: a candidate among the two-sided rows a thread holds in its SECOND slot (r >= 256: the later acceleration rows, the pairs)"""
    def ok(c, g):
        return c.lsc is None and any(((s["row"] - _n_lsc(c)) >> 1) >= T for s in _traced(O, c)[1])

    return SP._pick(O, SP._designed(O, M, dim), "a candidate in a thread's second two-sided slot", ok)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_later_passes_alternate_between_lsc_and_two_sided_minima_and_an_instance_without_lsc_rows(api, oracle, torch_cuda, shape):
    M, dim = shape
    spec = DC.spec_of(M, dim, "lsc")

    def make():
        no_rows = SP._pick(oracle, SP._designed(oracle, M, dim), "three steps without LSC rows", lambda c, g: c.lsc is None and g["steps"] >= 3)
        cases = [alternating_case(oracle, spec), no_rows, SP.quiet_case(oracle, spec)]
        if dim * (15 * M + M * (M - 1) // 2) > T:  # (csrc/lscqp_das.hpp: num_pairs)
            cases.append(second_slot_case(oracle, M, dim))
        return SP.make_batch(api, oracle, spec, cases)

    b = SP.batch(("rt registers",) + shape, make)
    assert (len(b.cases) == 4) == (shape == (10, 2)), (shape, len(b.cases))  # (255 two-sided rows at M5 in 3-D: one slot a thread)
    G = SP.every_form(api, oracle, torch_cuda, b)
    assert G["info"]["iterations"][0] >= 3 and G["info"]["iterations"][1] >= 3 and G["info"]["iterations"][2] == 0, G["info"]["iterations"]


# ---- the fused entry: every optional pointer null and not null, a launch of one -------------------------------------------------------------
def _call(api, torch, b, knobs, order=None, x_init=None, info=True):
    """PR._device_call with the optional pointers of the entry chosen by the caller"""
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    sol = api.Solver(b.desc)
    for k, v in knobs.items():
        sol.set_knob(k, v)
    n = len(b.hdr)
    d_x = torch.zeros(n * sol.nv, dtype=torch.float64, device=dev)
    d_obj = torch.zeros(n, dtype=torch.float64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_info = torch.zeros(n * np.dtype(api.INFO_DTYPE).itemsize, dtype=torch.uint8, device=dev) if info else None
    d_order = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    d_xi = None if x_init is None else torch.from_numpy(np.ascontiguousarray(x_init, dtype=np.float64)).to(dev)
    sol.solve_device(n, b.n_obs_max, up(b.hdr), up(b.rows), up(b.off), up(b.sfc), d_x, d_obj, d_st, d_info, d_x_init=d_xi, d_order=d_order)
    torch.cuda.synchronize()
    out = dict(x=d_x.cpu().numpy().reshape(n, -1), obj=d_obj.cpu().numpy(), status=d_st.cpu().numpy())
    if info:
        out["info"] = d_info.cpu().numpy().view(api.INFO_DTYPE)
    return out


def _same_fields(a, b, fields):
    return all(np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)) for f in fields)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_fused_entry_with_each_optional_pointer_null_and_not_null(api, oracle, torch_cuda, shape):
    """order (a non-identity permutation), row_offsets, the corridor boxes, x_init and info_out, each absent and present, and a launch
    of one instance.  (The batch's refused instance -- one obstacle beyond the capacity -- is the one whose x depends on x_init.)"""
    M, dim = shape
    cap = PR.capacity_of(api, M, dim)
    plain = PR.batch(("mixed",) + shape, PR.mixed_counts, api, oracle, M, dim, cap)
    G = PR.every_form(api, oracle, torch_cuda, plain)  # (row_offsets and boxes present, the rest absent; the oracle's bars)
    n, perm = len(plain.hdr), [5, 2, 7, 0, 3, 6, 1, 4]
    xi = np.random.RandomState(3).randn(n, G["x"].shape[1])
    ok = np.arange(n) != plain.expect.index(PR.CAPACITY)
    R = [_call(api, torch_cuda, plain, knobs, order=perm, x_init=xi, info=True) for _, knobs in FORMS[:2]]
    N = [_call(api, torch_cuda, plain, knobs, order=perm, x_init=xi, info=False) for _, knobs in FORMS[:2]]
    assert _same_fields(R[0], R[1], ("x", "obj", "status", "info")) and _same_fields(N[0], N[1], ("x", "obj", "status"))  # new text against old
    assert _same_fields(N[0], R[0], ("x", "obj", "status"))  # nothing but the record depends on info_out
    assert _same_fields({f: R[0][f][ok] for f in R[0]}, {f: G[f][ok] for f in G}, ("x", "obj", "status", "info"))  # nor what the phase finishes on x_init or the order
    assert np.array_equal(R[0]["status"], G["status"])
    assert _kernel_launches(api, torch_cuda, plain, FORMS[0][1]) == 1
    for key, kw in ((("no rows",) + shape, dict(with_rows=False)), (("no sfc",) + shape, dict(use_sfc=False)), (("one",) + shape, dict(order=[0], n=1))):
        b = PR.batch(key, PR.mixed_counts, api, oracle, M, dim, cap, **kw)
        PR.every_form(api, oracle, torch_cuda, b)
