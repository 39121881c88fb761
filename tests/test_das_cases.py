"""The designed instances of tests/das_cases.py and the numpy restatement of the dual active-set phase (tests/das_reference.py), on the CPU.

What tests/test_das_families_gpu.py asks of the device -- every case finished by the phase ALONE, in exactly the restatement's number of
steps -- rests on what is shown here without a GPU:
  premises      the oracle calls every case OPTIMAL, the rows that carry a multiplier at its optimum include the family, axis, side and
                segment the case is named for (classified by the structure of the assembled row), and there are at most 12 of them: what
                the launch policy's comment calls the most any feasible instance of its sweeps needed;
  restatement   its optimum is the polished oracle's within 1e-8 m and 1e-8 relative in the objective, its final active set is the oracle's;
  budgets       at most 20 rows held at once and 48 steps on every case: the policy's "small" budgets, so that no hand-over is legitimate;
  margins       at most 10 % of the cases decide a selection or a ratio test by less than 1e-6 m (the GPU test leaves those out of its
                step-count comparison);
  leaving rows  at least six cases drop a row, with a leaving row in the first, a middle and the last position of the active list."""
import numpy as np
import pytest

from tests import das_cases as DC

X_TOL, OBJ_TOL = 1e-8, 1e-8
MAX_ACTIVE, MAX_HELD, MAX_STEPS = DC.MAX_ACTIVE, 20, 48
CLEAR_MARGIN = 1e-6  # metres: three orders above the kernel's 1e-9 m bar; a selection condition of the step-count comparison, not a tolerance
SHAPE_IDS = ["M%dd%d%s" % s for s in DC.SHAPES]


def restated(oracle, case):
    if not hasattr(case, "das"):
        case.das = DC.restate(oracle, case)
    return case.das


def _sfc(oracle, c):
    return c.sfc if c.sfc is not None else DC.wide_box(oracle, c.spec)


@pytest.mark.parametrize("shape", DC.SHAPES, ids=SHAPE_IDS)
def test_premises_of_the_designed_cases(oracle, shape):
    cases = DC.cases(oracle, *shape)
    names = {c.name.split("_k")[0].split("_m")[0].split("_slot")[0].split("_ts")[0].split("_v")[0] for c in cases}
    want = {"vel", "acc_push", "acc_brake", "corridor", "range", "waypoint", "lsc", "lsc_oblique", "terminal", "degenerate_plane_twice", "degenerate_face_on_plane"}
    want |= {"world"} | ({"pair", "leaving"} if shape[0] >= 5 else set()) | ({"rsfc_ceiling_binds_in_lsc", "rsfc_ceiling_relaxed"} if shape[1:] == (3, "lsc") else set())
    assert want <= names, want - names
    assert len(cases) <= 256
    for c in cases:
        r = c.oracle
        assert r["status"] == 0, c
        rows = c.rows
        assert len(rows) <= MAX_ACTIVE, (c, len(rows))
        if c.expect is None:
            continue
        if c.expect["family"] is None:  # PLANNER_RSFC: z of segment 0 above the world's ceiling, and no row holds it
            z = r["x"].reshape(c.spec["dim"], c.spec["M"], 6)[2]
            assert z[0, 3:5].max() > c.expect["above"] + 1e-4 and z[1:].max() <= c.expect["above"] + 1e-9
            assert not any(w["family"] == "interval" and w["axis"] == 2 and w["segment"] == 0 for w in rows), c
            continue
        assert any(DC.matches(c.expect, w) for w in rows), (c, c.expect, [(w["family"], w["axis"], w["side"], w["segment"], w["bound"]) for w in rows])
        if "ts" in c.expect:
            assert oracle.terminal_segments(DC.oracle_class(oracle, c.spec), c.agent) == c.expect["ts"]
    # the terminal-segment slabs: 1, M and (from M = 4 up) one value between
    ts = {c.expect["ts"] for c in cases if c.expect and "ts" in c.expect}
    M = shape[0]
    assert {1, M} <= ts and (M < 4 or any(1 < t < M for t in ts)), ts
    # both sides of a two-sided row, every axis (z included in 3-D), for the interval, velocity and acceleration families
    for fam in ("interval", "velocity", "acceleration", "range"):
        seen = {(c.expect["axis"], c.expect["side"]) for c in cases if c.expect and c.expect["family"] == fam and c.group == "main"}
        assert {(k, s) for k in range(shape[1]) for s in (0, 1)} <= seen, (fam, seen)
    if M >= 5:
        assert {c.expect["axis"] for c in cases if c.expect and c.expect["family"] == "pair"} == set(range(shape[1]))


@pytest.mark.parametrize("shape", DC.SHAPES, ids=SHAPE_IDS)
def test_restatement_against_the_oracle_and_inside_the_small_budgets(oracle, shape):
    for c in DC.cases(oracle, *shape):
        r, g = c.oracle, restated(oracle, c)
        assert g["status"] == "optimal", (c, g["status"], g["steps"])
        assert g["peak"] <= MAX_HELD and g["steps"] <= MAX_STEPS, (c, g["peak"], g["steps"])
        assert np.abs(g["x"] - r["x"]).max() <= X_TOL, (c, np.abs(g["x"] - r["x"]).max())
        A = oracle.assemble(DC.oracle_class(oracle, c.spec), c.agent, c.lsc, _sfc(oracle, c))
        # (the objective of the POLISHED point through the assembled model: the oracle's own figure is its interior-point iterate's and carries
        # that iterate's gap -- a few 1e-8 relative on the M = 12 ceiling case)
        obj, ref = DC.objective(A, g["x"]), DC.objective(A, r["x"])
        assert abs(obj - ref) <= OBJ_TOL * max(1.0, abs(ref)), (c, obj, ref, r["obj"])
        assert abs(ref - r["obj"]) <= 1e-6 * max(1.0, abs(ref)), (c, ref, r["obj"])
        own, theirs = DC.signatures(c.spec, DC.restated_vectors(c.spec, g)), DC.signatures(c.spec, [w["vec"] for w in c.rows])
        # The active set is the oracle's -- where the multipliers are unique.  Rows the equality rows make dependent (a velocity row between
        # two held ones across a junction: continuity ties the three) share their multipliers in any proportion: the interior-point oracle
        # spreads them, an active-set method holds a basis.  There the restatement's rows must be among the rows that are tight at the
        # oracle's optimum, and span the oracle's.
        tight = DC.signatures(c.spec, DC.tight_vectors(oracle, c, r["x"]))
        assert own <= tight, (c, len(own - tight))
        if DC.independent(theirs):
            assert own == theirs, (c, len(own), len(theirs))
        else:
            assert DC.rank(own | theirs) == DC.rank(own) == len(own), (c, len(own), len(theirs))


def test_few_cases_decide_a_step_by_less_than_the_clear_margin(oracle):
    allc = [c for s in DC.SHAPES for c in DC.cases(oracle, *s)]
    unclear = [c for c in allc if not restated(oracle, c)["margin"] > CLEAR_MARGIN]
    print("%d cases, %d below the clear margin: %s" % (len(allc), len(unclear), [(c.key, c.name, "%.1e" % c.das["margin"]) for c in unclear]))
    assert len(unclear) <= 0.10 * len(allc), (len(unclear), len(allc))


def test_rows_leave_from_the_first_a_middle_and_the_last_position(oracle):
    allc = [c for s in DC.SHAPES for c in DC.cases(oracle, *s)]
    left = [(c, restated(oracle, c)["left"]) for c in allc if restated(oracle, c)["left"]]
    assert len(left) >= 6, len(left)
    pos = {("first" if l == 0 else "last" if l == kk - 1 else "middle") for _, ls in left for (l, kk) in ls if kk >= 2}
    assert pos == {"first", "middle", "last"}, pos
    # ... on the shapes with a fused form too (their carve of J and W is another: compile-time)
    assert {c.key for c, ls in left if any(kk >= 2 for _, kk in ls)} >= set(DC.FUSED_SHAPES)
