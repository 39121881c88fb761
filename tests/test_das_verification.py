"""The fused phase's row slots sized to its rows, and its verification as straight-line code (csrc/lscqp_fused.hip: kU; csrc/lscqp_das_body.inc:
finish_local in the latency text, LSCQP_DAS_FORM LSCQP_DAS_LATENCY) -- on the inputs at which a slot, a clamped index or the multipliers' array can go
wrong: a cutting plane whose candidate rows lie in the first slot, across the boundaries between the slots (ids 255 | 256 and 511 | 512) and
in the last rows the three slots cover; obstacle counts that fill two slots, three, the capacity and one more; an instance without rows
between two that step; and verifications that read multipliers -- one and two rows held, a row that left, an LSC row beside a two-sided
one.

Batches of at most 8 instances, each through the four forms of tests/test_das_prologue.py: the fused launch runs the new text at M5 in 3-D
and at M10 in 2-D, the two launches and the one- and two-wavefront forms the old one, so "the same bytes in every form" compares new with
old.  The cases at M5 in 3-D are the slots' and the multipliers'; those at M10 in 2-D end with an LSC row held, whose third entry (axis 2,
coefficient 0) addresses the word behind the multipliers' array there (NOTES.md section 24, D).  Every instance expected OPTIMAL is finished by the phase in the CPU
restatement's step count (tests/das_reference.py) and held to the polished CPU oracle at 1e-8 m / 1e-8 relative; the builders assert
their premises on the CPU."""
import numpy as np
import pytest

from tests import das_cases as DC
from tests import test_das_step_path as SP
from tests.test_das_prologue import FORMS, _device_call, _same, capacity_of

pytestmark = pytest.mark.gpu

X_TOL, OBJ_TOL = 1e-8, 1e-8  # tests/test_das_families_gpu.py
OPTIMAL, CAPACITY = "optimal", "capacity"
OBLIQUE = [-0.75, 0.5, 0.25]
PLANES = [(0, 0), (8, 2), (17, 0), (19, 4)]  # (obstacle, segment) of the one cutting plane among 20 obstacles at M5
PLANE_IDS = [(0, 6), (252, 258), (510, 516), (594, 600)]  # the ids of that record's six rows
COUNTS = [17, 18, 20, 21]  # 510 rows (two slots of 256 and two rows), 540, the capacity's 600, and an instance the phase refuses


# ---- instances, premises asserted with the restatement ----------------------------------------------------------------------------------
def one_plane(O, spec, n_obs, oi, m, name):
    """test_das_step_path.plane_case with one cutting plane at (obstacle oi, segment m): one step, onto a row of that record"""
    M, dim = spec["M"], spec["dim"]
    c = SP.plane_case(O, spec, n_obs, [(oi, m, OBLIQUE if dim == 3 else [-0.75, 0.5, 0.0], 0.6)], seed=200 + 31 * oi + m, name=name)
    g = SP.restated(O, c)
    lo = (oi * M + m) * 6
    assert g["status"] == "optimal" and g["steps"] == 1 and len(g["active"]) == 1 and lo + 3 <= g["active"][0][0] < lo + 6, (name, g["steps"], g["active"])
    return c


def position_cases(O, spec, cap):
    assert spec["M"] == 5 and cap == 20
    out = [one_plane(O, spec, cap, oi, m, "plane_at_%d_%d" % (oi, m)) for (oi, m) in PLANES]
    for c, (lo, hi), (oi, m) in zip(out, PLANE_IDS, PLANES):
        assert lo == (oi * spec["M"] + m) * 6 and lo <= SP.restated(O, c)["active"][0][0] < hi
    # (the record of the second plane lies across ids 255 | 256, the third's across 511 | 512, the last's ends at the carve's last row)
    assert PLANE_IDS[1][0] < 256 < PLANE_IDS[1][1] and PLANE_IDS[2][0] < 512 < PLANE_IDS[2][1] and PLANE_IDS[3][1] == cap * 6 * spec["M"]
    return out


def count_cases(O, spec, cap):
    """the plane in the LAST obstacle; the instance beyond the capacity has the capacity's rows and claims one obstacle more"""
    assert COUNTS[-2] == cap and COUNTS[-1] == cap + 1
    return [one_plane(O, spec, min(k, cap), min(k, cap) - 1, spec["M"] // 2, "plane_last_of_%d" % k) for k in COUNTS]


def lsc_and_face_case(O, spec):
    """an LSC row and a two-sided row held together: the cutting plane of one_plane on the middle segment and a corridor face across the
    way on the last one -- the first choice of the face's position at which the restatement holds exactly one row of each kind"""
    M, dim = spec["M"], spec["dim"]
    n_obs = 3
    base = SP.plane_case(O, spec, n_obs, [(1, M // 2, OBLIQUE if dim == 3 else [-0.75, 0.5, 0.0], 0.6)], seed=77, name="lsc_and_face")
    a = SP._lsc_agent(spec)
    free = DC._free(O, spec, **a)
    for m in (M - 1, 1, M // 2):
        for frac in (0.6, 0.4, 0.8, 0.2):
            box = DC.wide_box(O, spec)
            box["bmax"][m][0] = a["p0"][0] + frac * np.abs(free[0][m]).max()
            c = DC.Case("lsc_and_face_m%d_%g" % (m, frac), spec, base.agent, lsc=base.lsc, sfc=box)
            g = SP.restated(O, c)
            ids = sorted(r[0] for r in g["active"])
            if g["status"] == "optimal" and len(ids) == 2 and ids[0] < n_obs * 6 * M <= ids[1] and g["margin"] > 1e-6:
                return c
    raise AssertionError("no face holds one LSC row and one two-sided row")


def multiplier_cases(O, spec):
    """verifications that read A'u: one row held (an LSC row), two rows held, a row that left on the way, an LSC row beside a two-sided one"""
    M = spec["M"]
    one = one_plane(O, spec, 3, 1, M // 2, "one_lsc_row_held")
    two = SP.held_case(O, spec, 2)
    left = SP.leaving_cases(O, spec)[0]
    both = lsc_and_face_case(O, spec)
    g = [SP.restated(O, c) for c in (one, two, left, both)]
    assert len(g[0]["active"]) == 1 and len(g[1]["active"]) == 2 and g[2]["left"] and len(g[2]["active"]) >= 1 and len(g[3]["active"]) == 2
    assert all(x["status"] == "optimal" for x in g)
    return [one, two, left, both]


def lsc_row_cases_2d(O, spec):
    """M10 in 2-D: instances that end with an LSC row held (its third entry: axis 2, coefficient 0) -- alone after one step, among other
    rows after several, and beside a corridor face"""
    M = spec["M"]
    nrm = [-0.75, 0.5, 0.0]
    out = [one_plane(O, spec, 2, 1, M // 2, "lsc_row_2d_mid"), SP.plane_case(O, spec, 3, [(0, M - 1, nrm, 0.6)], seed=293, name="lsc_row_2d_last"),
           lsc_and_face_case(O, spec)]
    for c in out:
        g = SP.restated(O, c)
        assert g["status"] == "optimal" and g["margin"] > 1e-6 and any(r[0] < int(c.agent["n_obs"]) * 6 * M for r in g["active"]), (c.name, g["steps"], g["active"])
    assert SP.restated(O, out[1])["steps"] > 1
    return out


# ---- the batch through every form -----------------------------------------------------------------------------------------------------
def every_form(api, O, torch, b):
    """the same bytes from every form; every OPTIMAL instance by the phase, in the restatement's steps, at the oracle's optimum"""
    res = [(name, _device_call(api, torch, b, knobs)) for name, knobs in FORMS]
    G = res[0][1]
    for name, r in res[1:]:
        assert _same(r, G), (name, r["status"], G["status"], r["info"], G["info"])
    if b.ref is None:
        b.ref = {}
        for q, e in enumerate(b.expect):
            if e == OPTIMAL:
                r = O.solve(b.ocls, b.agents[q], b.lscs[q], b.boxes[q])
                assert r["status"] == 0, ("the oracle solves every feasible instance", q, b.cases[q].name)
                b.ref[q] = (r["x"], DC.objective(O.assemble(b.ocls, b.agents[q], b.lscs[q], b.boxes[q]), r["x"]))
    info = G["info"]
    for q, e in enumerate(b.expect):
        if e == CAPACITY:
            assert G["status"][q] == api.STATUS_CAPACITY, (q, G["status"][q])
            continue
        xr, fr = b.ref[q]
        g = SP.restated(O, b.cases[q])
        dx, dobj = np.abs(G["x"][q] - xr).max(), abs(G["obj"][q] - fr) / max(1.0, abs(fr))
        print("verification| instance %d %s: %d steps (restatement %d, margin %.1e m), |dx| %.1e m, objective %.1e rel, res_dual %.1e"
              % (q, b.cases[q].name, info["iterations"][q], g["steps"], g["margin"], dx, dobj, info["res_dual"][q]))
        assert G["status"][q] == api.STATUS_OPTIMAL and (info["flags"][q] & api.INFO_ACTIVE_SET), (q, G["status"][q], info[q])
        assert dx <= X_TOL and dobj <= OBJ_TOL, (q, dx, dobj)
        if g["margin"] > 1e-6:
            assert info["iterations"][q] == g["steps"], (q, b.cases[q].name, info["iterations"][q], g["steps"])
    return G


_BATCHES = {}


def batch(key, make):
    if key not in _BATCHES:
        _BATCHES[key] = make()
    return _BATCHES[key]


def test_a_cutting_plane_in_the_first_slot_across_both_slot_boundaries_and_in_the_last_rows(api, oracle, torch_cuda):
    spec = DC.spec_of(5, 3, "lsc")
    cap = capacity_of(api, 5, 3)
    b = batch("positions", lambda: SP.make_batch(api, oracle, spec, position_cases(oracle, spec, cap)))
    assert list(b.hdr["n_obs"]) == [cap] * 4
    G = every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"] == 1).all() and np.isfinite(G["x"]).all()


def test_obstacle_counts_of_two_and_three_slots_the_capacity_and_one_more(api, oracle, torch_cuda):
    spec = DC.spec_of(5, 3, "lsc")
    cap = capacity_of(api, 5, 3)

    def make():
        b = SP.make_batch(api, oracle, spec, count_cases(oracle, spec, cap), expect=[OPTIMAL] * 3 + [CAPACITY])
        b.hdr["n_obs"][3] = cap + 1  # (it claims one obstacle more than it has rows: none of them may be read)
        b.n_obs_max = cap
        return b

    b = batch("counts", make)
    assert list(b.hdr["n_obs"]) == COUNTS and [k * 30 for k in COUNTS[:3]] == [510, 540, 600]
    G = every_form(api, oracle, torch_cuda, b)
    assert (G["info"]["iterations"][:3] == 1).all() and np.isfinite(G["x"]).all() and np.isfinite(G["obj"]).all()


def test_an_instance_without_rows_between_two_that_step(api, oracle, torch_cuda):
    spec = DC.spec_of(5, 3, "lsc")
    cap = capacity_of(api, 5, 3)

    def make():
        first = one_plane(oracle, spec, cap, cap - 1, 4, "stepper_last_rows")
        none = SP.quiet_case(oracle, spec)
        assert int(none.agent["n_obs"]) == 0
        return SP.make_batch(api, oracle, spec, [first, none, one_plane(oracle, spec, 9, 8, 2, "stepper_across_256")])

    b = batch("zero", make)
    assert list(b.hdr["n_obs"]) == [cap, 0, 9]
    G = every_form(api, oracle, torch_cuda, b)
    assert list(G["info"]["iterations"]) == [1, 0, 1]


def test_a_verification_with_one_and_two_multipliers_a_row_that_left_and_an_lsc_row_beside_a_two_sided_one(api, oracle, torch_cuda):
    spec = DC.spec_of(5, 3, "lsc")
    b = batch("multipliers", lambda: SP.make_batch(api, oracle, spec, multiplier_cases(oracle, spec)))
    G = every_form(api, oracle, torch_cuda, b)
    assert G["info"]["iterations"][0] == 1 and G["info"]["iterations"][1] == 2 and (G["info"]["res_dual"] <= 1e-9).all()


def test_an_active_lsc_row_in_two_dimensions_addresses_the_word_behind_the_multipliers(api, oracle, torch_cuda):
    spec = DC.spec_of(10, 2, "lsc")
    b = batch("lsc_2d", lambda: SP.make_batch(api, oracle, spec, lsc_row_cases_2d(oracle, spec)))
    every_form(api, oracle, torch_cuda, b)
