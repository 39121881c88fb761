"""What a solve call launches, pinned on no device: Solver.solve_plan runs the planner the solve worker runs (csrc/lscqp_solve_plan.hpp) with
the CU count as an argument (256 throughout).  Expected values are literals: the phase's launch shapes and LDS footprints at every
threshold of the policy and along its give-up order, every knob override, and the chain of passes per kind of call as
(kind, repair, scan, queue counter, reads x_init) -- with (slots, waves, mixed) of the kernel instance where the case is about it."""
import ctypes as C
import itertools

import pytest

NCU = 256
LDS_LIMIT = 163840
PHASE = ("threads", "kmax", "steps", "cacheC", "stage_rows", "screen")


def _solver(api, knobs=(), prescreen=False, **desc):
    s = api.Solver(api.make_desc(**desc))
    for k, v in knobs:
        s.set_knob(k, v)
    if prescreen:
        s.set_prescreen(api.PRESCREEN_ON)
    return s


def _phase(plan):
    ph = [p for p in plan["passes"] if p["kind"] == "phase"]
    assert len(ph) <= 1
    return ph[0] if ph else None


def _shape(plan):
    ph = _phase(plan)
    return None if ph is None else tuple(ph[k] for k in PHASE) + (ph["lds_bytes"],)


def _chain(plan, inst=False):
    assert plan["error"] is None, plan
    return [(p["kind"], p["repair"], p["scan"], p["queue"], p["x_init"]) + (((p["slots"], p["waves"], p["mixed"]),) if inst else ()) for p in plan["passes"]]


def _lds(api, M, dim, kmax, cacheC, stage_rows):
    f = api.lib().lscqp_das_lds_bytes
    f.restype, f.argtypes = C.c_size_t, [C.c_int] * 5
    return f(M, dim, kmax, cacheC, stage_rows)


# ---- the phase's launch shape ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, want", [
    # n -> threads, kmax, steps, cacheC, stage_rows, screen (bit 1: the first look inside the loop), footprint
    (256, (256, 32, 96, 1, 600, 2, 69360)),
    (257, (256, 20, 48, 1, 600, 2, 54864)),
    (512, (256, 20, 48, 1, 600, 2, 54864)),
    (513, (256, 8, 24, 0, 0, 0, 16272)),
    (2048, (256, 8, 24, 0, 0, 0, 16272)),
    (2049, (64, 8, 24, 0, 0, 0, 16272)),
])
def test_phase_shape_at_the_batch_size_thresholds(api, n, want):
    s = _solver(api, M=5, dim=3)
    assert _shape(s.solve_plan(n, 20, n_cu=NCU)) == want
    assert _lds(api, 5, 3, want[1], want[3], want[4]) == want[6]


@pytest.mark.parametrize("M, dim, n_obs, n, kmax, steps, stage_rows, lds", [
    (10, 3, 30, 256, 32, 96, 1800, 162128),  # fits
    (10, 3, 31, 256, 20, 96, 1860, 140912),  # the retreat: 20 rows rather than lose the staged rows
    (10, 3, 40, 256, 20, 96, 2400, 158192),  # (the step budget stays that of a batch of n <= CUs)
    # THE RETREAT QUIRK (csrc/lscqp_solve_plan.hpp): the staged rows do not fit beside 32 rows and are given up; 32 rows then fit at
    # 104 528 B, but the retreat rule tests the footprint WITH the staged rows it has just given up, cuts to 20, and the staged rows do not
    # fit beside 20 either.  Pinned as it is; a change of the policy decides whether it stays.
    (10, 3, 64, 256, 20, 96, 0, 81392),
    (10, 2, 24, 256, 32, 96, 1440, 129888),
    (10, 3, 64, 257, 20, 48, 0, 81392),
])
def test_phase_shape_along_the_lds_give_up_order(api, M, dim, n_obs, n, kmax, steps, stage_rows, lds):
    s = _solver(api, M=M, dim=dim)
    assert _shape(s.solve_plan(n, n_obs, n_cu=NCU)) == (256, kmax, steps, 1, stage_rows, 2, lds)
    assert _lds(api, M, dim, kmax, 1, stage_rows) == lds


def test_the_quirk_gives_up_rows_that_would_fit(api):
    assert _lds(api, 10, 3, 32, 1, 0) == 104528 <= LDS_LIMIT < _lds(api, 10, 3, 20, 1, 64 * 60)


def test_without_staged_rows_every_accepted_shape_fits(api):
    """Why the `give up the table copy` branch and the loop over kmax cannot fire under the default policy."""
    worst = max(_lds(api, M, dim, 32, 1, 0) for M in range(2, 13) for dim in (2, 3))
    assert worst == _lds(api, 12, 3, 32, 1, 0) == 130704 <= LDS_LIMIT


@pytest.mark.parametrize("knob, value, field, want", [
    ("das_threads", 64, "threads", 64), ("das_kmax", 12, "kmax", 12), ("das_steps", 7, "steps", 7), ("das_cache", 0, "cacheC", 0),
    ("das_stage", 0, "stage_rows", 0), ("das_screen", 1, "screen", 3), ("das_loop", 0, "screen", 0),
])
def test_a_knob_override_replaces_its_own_field_only(api, knob, value, field, want):
    base = _phase(_solver(api, M=5, dim=3).solve_plan(64, 20, n_cu=NCU))
    got = _phase(_solver(api, [(knob, value)], M=5, dim=3).solve_plan(64, 20, n_cu=NCU))
    assert got[field] == want != base[field]
    for k in PHASE:
        if k != field:
            assert got[k] == base[k], (knob, k)


def test_das_kmax_set_disables_the_retreat_rule(api):
    s = _solver(api, [("das_kmax", 32)], M=10, dim=3)
    assert _shape(s.solve_plan(256, 40, n_cu=NCU)) == (256, 32, 96, 1, 0, 2, 104528)  # (the staged rows go instead)


# ---- the chain -------------------------------------------------------------------------------------------------------------------------

FUSED = [("fused", 3, 0, 0), ("phase", 0, 0, 0), ("instance", 3, 0, 0)]  # + reads x_init; the fused pass, then the two it stands for


def _fused(x):
    return [p + (x,) for p in FUSED]


@pytest.mark.parametrize("retry, x_init, behind", [
    (0, 0, []), (0, 1, []),
    (1, 0, []), (1, 1, [("instance", 1, 0, 0, 0)]),
    (2, 0, [("generic", 2, 0, 0, 0)]), (2, 1, [("instance", 1, 0, 0, 0), ("generic", 2, 0, 0, 0)]),  # (M = 5 has no other-order instance)
    (3, 0, [("generic", 2, 0, 0, 0)]), (3, 1, [("instance", 1, 0, 0, 0), ("generic", 2, 0, 0, 0)]),
])
def test_chain_of_a_c1_class_call(api, retry, x_init, behind):
    plan = _solver(api, M=5, dim=3).solve_plan(64, 20, retry=retry, has_x_init=x_init, n_cu=NCU)
    assert _chain(plan) == _fused(x_init) + behind
    assert [p["what"] for p in plan["passes"]][:3] == ["fused active-set phase", "dual active-set phase", ""]
    assert all((p["slots"], p["waves"], p["mixed"]) == (5, 2, 0) for p in plan["passes"] if p["kind"] in ("fused", "instance"))


CHAINS = {
    # beyond the CU count: two launches, and the second pass (not the near-empty first one behind the phase) gets a queue counter
    "n257": (dict(M=5, dim=3), (), dict(n=257, retry=1, has_x_init=1),
             [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 0, 0, 1, (5, 2, 0)), ("instance", 1, 0, 1, 0, (5, 2, 0))]),
    # a batch that fills the chip takes the one-wavefront instance, which has no persistent form: no counter
    "n2049": (dict(M=5, dim=3), (), dict(n=2049, retry=1, has_x_init=1),
              [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 0, 0, 1, (10, 1, 0)), ("instance", 1, 0, 0, 0, (10, 1, 0))]),
    "n2049_persistent": (dict(M=10, dim=3), (), dict(n=2049, n_obs=40, retry=1, has_x_init=1),
                         [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 0, 0, 1, (10, 4, 0)), ("instance", 1, 0, 1, 0, (10, 4, 0))]),
    "n2049_persistent_phase_off": (dict(M=10, dim=3), (("active_set_off", 1),), dict(n=2049, n_obs=40, retry=1, has_x_init=1),
                                   [("instance", 0, 0, 1, 1, (10, 4, 0)), ("instance", 1, 0, 1, 0, (10, 4, 0))]),
    "no_queue": (dict(M=10, dim=3), (("active_set_off", 1), ("no_queue", 1)), dict(n=2049, n_obs=40, retry=1, has_x_init=1),
                 [("instance", 0, 0, 0, 1, (10, 4, 0)), ("instance", 1, 0, 0, 0, (10, 4, 0))]),
    # mixed precision behind the phase: straight to the fp64 instance, one launch instead of two
    "mixed": (dict(M=5, dim=3, precision="mixed"), (), dict(n=64, retry=0, has_x_init=1),
              [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 0, 0, 1, (5, 2, 0))]),
    "mixed_retry": (dict(M=5, dim=3, precision="mixed"), (), dict(n=64, retry=1, has_x_init=1),
                    [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 0, 0, 1, (5, 2, 0)), ("instance", 1, 0, 0, 0, (5, 2, 0))]),
    # ... without the phase: float32 first, the fp64 instance re-solves from the same start
    "mixed_phase_off": (dict(M=5, dim=3, precision="mixed"), (("active_set_off", 1),), dict(n=64, retry=0, has_x_init=1),
                        [("instance", 0, 0, 0, 1, (10, 1, 1)), ("instance", 1, 0, 0, 1, (5, 2, 0))]),
    "force_generic": (dict(M=5, dim=3), (("force_generic", 1),), dict(n=64, retry=3, has_x_init=1),
                      [("phase", 0, 0, 0, 1, (0, 0, 0)), ("generic", 3, 0, 0, 1, (0, 0, 0)), ("generic", 1, 0, 0, 0, (0, 0, 0)), ("generic", 2, 0, 0, 0, (0, 0, 0))]),
    "force_generic_cold_retry": (dict(M=5, dim=3), (("force_generic", 1),), dict(n=64, retry=1, has_x_init=0),
                                 [("phase", 0, 0, 0, 0, (0, 0, 0)), ("generic", 3, 0, 0, 0, (0, 0, 0))]),
    "M11_no_compiled_instance": (dict(M=11, dim=3), (), dict(n=64, retry=2, has_x_init=1),
                                 [("phase", 0, 0, 0, 1, (0, 0, 0)), ("generic", 3, 0, 0, 1, (0, 0, 0)), ("generic", 1, 0, 0, 0, (0, 0, 0)), ("generic", 2, 0, 0, 0, (0, 0, 0))]),
    "active_set_only": (dict(M=5, dim=3, active_set="only"), (), dict(n=64, retry=3, has_x_init=1), [("phase", 0, 0, 0, 1, (0, 0, 0))]),
    "active_set_off": (dict(M=5, dim=3, active_set="off"), (), dict(n=64, retry=1, has_x_init=1),
                       [("instance", 0, 0, 0, 1, (5, 2, 0)), ("instance", 1, 0, 0, 0, (5, 2, 0))]),
    # the scan form behind the phase: both passes on the persistent fp64 instance of equal capacity, no counter, no fused launch
    "behind_scan": (dict(M=5, dim=3), (("behind_scan", 1),), dict(n=64, retry=1, has_x_init=1),
                    [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 1, 0, 1, (5, 2, 0)), ("instance", 1, 1, 0, 0, (5, 2, 0))]),
    "behind_scan_large": (dict(M=5, dim=3), (("behind_scan", 1),), dict(n=2049, retry=1, has_x_init=1),
                          [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 1, 0, 1, (5, 2, 0)), ("instance", 1, 1, 0, 0, (5, 2, 0))]),
    "behind_scan_mixed": (dict(M=5, dim=3, precision="mixed"), (("behind_scan", 1),), dict(n=2049, retry=1, has_x_init=1),
                          [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 1, 0, 1, (5, 2, 0)), ("instance", 1, 1, 0, 0, (5, 2, 0))]),
    "das_fused_0": (dict(M=5, dim=3), (("das_fused", 0),), dict(n=64, retry=1, has_x_init=1),
                    [("phase", 0, 0, 0, 1, (0, 0, 0)), ("instance", 3, 0, 0, 1, (5, 2, 0)), ("instance", 1, 0, 0, 0, (5, 2, 0))]),
    # retry = 2 on a shape that has both elimination orders (forest10 replica): the second pass on the other one, also for a cold batch
    "other_order_second_pass": (dict(M=10, dim=2), (), dict(n=10, n_obs=9, retry=2, has_x_init=0),
                                [("fused", 3, 0, 0, 0, (5, 2, 0)), ("phase", 0, 0, 0, 0, (0, 0, 0)), ("instance", 3, 0, 0, 0, (5, 2, 0)),
                                 ("instance", 1, 0, 0, 0, (10, 1, 0)), ("generic", 2, 0, 0, 0, (0, 0, 0))]),
    # the parts the host-pointer entries and the sharded solve run after looking at the statuses
    "part_behind_phase": (dict(M=5, dim=3), (), dict(n=64, retry=1, has_x_init=1, part="behind"),
                          [("instance", 3, 0, 0, 1, (5, 2, 0)), ("instance", 1, 0, 0, 0, (5, 2, 0))]),
    "part_other_order": (dict(M=10, dim=2), (), dict(n=10, n_obs=9, part="other"), [("instance", 1, 0, 0, 0, (10, 1, 0))]),
    "part_other_order_without_one": (dict(M=5, dim=3), (), dict(n=64, part="other"), []),
    "part_other_order_run_time_shaped": (dict(M=11, dim=3), (), dict(n=64, part="other"), []),
    "part_rescue": (dict(M=5, dim=3), (), dict(n=64, part="rescue"), [("generic", 2, 0, 0, 0, (0, 0, 0))]),
    "part_rescue_run_time_shaped": (dict(M=11, dim=3), (), dict(n=64, part="rescue"), [("generic", 2, 0, 0, 0, (0, 0, 0))]),
    "part_rescue_active_set_only": (dict(M=5, dim=3, active_set="only"), (), dict(n=64, part="rescue"), []),
    # no tables on the device: no phase, and the first pass solves everything
    "tables_unavailable": (dict(M=5, dim=3), (), dict(n=64, retry=0, has_x_init=1, tables_available=0), [("instance", 0, 0, 0, 1, (5, 2, 0))]),
}


def _plan_of(api, desc, knobs, call, prescreen=False):
    desc = dict(desc)
    if "precision" in desc:
        desc["precision"] = api.PRECISION_MIXED
    if "active_set" in desc:
        desc["active_set"] = {"only": api.ACTIVE_SET_ONLY, "off": api.ACTIVE_SET_OFF}[desc["active_set"]]
    call = dict(call)
    part = {"whole": api.PLAN_WHOLE, "behind": api.PLAN_BEHIND_PHASE, "other": api.PLAN_OTHER_ORDER, "rescue": api.PLAN_RESCUE}[call.pop("part", "whole")]
    return _solver(api, knobs, prescreen, **desc).solve_plan(call.pop("n"), call.pop("n_obs", 20), part=part, n_cu=NCU, **call)


@pytest.mark.parametrize("case", list(CHAINS))
def test_chain(api, case):
    desc, knobs, call, want = CHAINS[case]
    plan = _plan_of(api, desc, knobs, call)
    assert _chain(plan, inst=True) == want
    assert not plan["deferred"]


def test_chain_with_the_prescreen_on(api):
    c1 = dict(M=5, dim=3)
    plan = _plan_of(api, c1, (), dict(n=64, retry=1, has_x_init=1), prescreen=True)
    assert _chain(plan) == [("prescreen", 0, 0, 0, 1), ("phase", 0, 0, 0, 1), ("instance", 3, 0, 0, 1), ("instance", 1, 0, 0, 0)]  # (fused is off)
    assert _phase(plan)["screen"] == 2 | 4  # bit 2: the phase skips what the prescreen proved
    # the first pass runs the way the pass behind the phase does even with the phase off ...
    plan = _plan_of(api, c1, (("active_set_off", 1),), dict(n=64, retry=0, has_x_init=1), prescreen=True)
    assert _chain(plan) == [("prescreen", 0, 0, 0, 1), ("instance", 3, 0, 0, 1)]
    # ... and in the part behind a phase that has run; the prescreen itself is not launched again
    plan = _plan_of(api, c1, (), dict(n=64, retry=1, has_x_init=1, part="behind"), prescreen=True)
    assert _chain(plan) == [("instance", 3, 0, 0, 1), ("instance", 1, 0, 0, 0)]
    # the single-pass parts know nothing of it
    assert _chain(_plan_of(api, c1, (), dict(n=64, part="rescue"), prescreen=True)) == [("generic", 2, 0, 0, 0)]


def test_deferred_plan_ends_behind_the_phase(api):
    plan = _plan_of(api, dict(M=5, dim=3), (), dict(n=64, retry=1, has_x_init=1, deferred=1))
    assert _chain(plan) == [("phase", 0, 0, 0, 1)] and plan["deferred"]  # (no fused launch for a caller that looks at the statuses first)
    # no phase, nothing to defer: the whole chain
    plan = _plan_of(api, dict(M=5, dim=3), (), dict(n=64, retry=1, has_x_init=1, deferred=1, tables_available=0))
    assert _chain(plan) == [("instance", 0, 0, 0, 1), ("instance", 1, 0, 0, 0)] and not plan["deferred"]


def test_calls_that_launch_nothing_say_why(api):
    assert _plan_of(api, dict(M=11, dim=3), (), dict(n=64, n_obs=500, retry=1)) == dict(passes=[], deferred=False, error="no_kernel", capacity=6)
    assert _plan_of(api, dict(M=5, dim=3, active_set="only"), (), dict(n=64, tables_available=0))["error"] == "only_without_phase"
    assert _plan_of(api, dict(M=5, dim=3), (("das_screen", 1),), dict(n=64), prescreen=True)["error"] == "lean_with_prescreen"


# ---- invariants over a sweep -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [2, 3])
def test_invariants_over_a_sweep(api, dim):
    for M in range(2, 13):
        s = _solver(api, M=M, dim=dim)
        cap = s.max_obstacles()
        for n_obs, n, retry, x_init in itertools.product(range(0, 65, 4), (256, 257, 512, 513, 2048, 2049), (0, 2), (0, 1)):
            plan = s.solve_plan(n, n_obs, retry=retry, has_x_init=x_init, n_cu=NCU)
            if n_obs > cap:
                assert plan["error"] == "no_kernel" and not plan["passes"]
                continue
            assert plan["error"] is None and len(plan["passes"]) <= plan["capacity"] == 6
            kinds = [p["kind"] for p in plan["passes"]]
            ph = _phase(plan)
            assert ph is not None and ph["lds_bytes"] <= LDS_LIMIT and ph["lds_bytes"] == _lds(api, M, dim, ph["kmax"], ph["cacheC"], ph["stage_rows"])
            if "fused" in kinds:
                assert n <= NCU and kinds[:3] == ["fused", "phase", "instance"]
            # behind a retry's second pass nothing starts from x_init again, and of the interior-point passes only the first does
            ip = [p for p in plan["passes"] if p["kind"] in ("instance", "generic")]
            assert sum(p["x_init"] for p in ip) == (1 if x_init else 0) and (not x_init or ip[0]["x_init"])
