"""The plan of a solve call (csrc/lscqp_solve_plan.hpp, Solver.solve_plan) against what the call enqueues: one solve_device call is captured
into a HIP graph, never launched, and its kernel nodes are counted.  The expectation is written from the plan, computed with the device's
real CU count: a plan that holds a fused pass also holds the phase and the first pass that replace it when the fused launcher refuses the
budgets, so a call launches len(passes) - 2 kernels where the launcher accepts and len(passes) - 1 where it refuses."""
import numpy as np
import pytest

from tests.das_capture import _batch, _Dev, _kernel_nodes

_BATCHES = {}


def _c1(api):
    if "c1" not in _BATCHES:
        _BATCHES["c1"] = _batch(api, "c1")
    return _BATCHES["c1"]


def _expected(plan, fused_accepts=True):
    assert plan["error"] is None and not plan["deferred"], plan
    kinds = [p["kind"] for p in plan["passes"]]
    assert len(kinds) <= plan["capacity"]
    if "fused" in kinds:
        k = kinds.index("fused")
        assert kinds[k + 1:k + 3] == ["phase", "instance"], kinds
        return len(kinds) - (2 if fused_accepts else 1)
    return len(kinds)


def _captured_and_planned(api, torch, sol, n, n_obs, arrays, x0, retry):
    d = _Dev(torch, sol, n, n_obs, arrays, x0)
    d.retry = retry
    d.solve()  # (eager first: the class's tables and the counter ring exist before the capture)
    d.result()
    d.clear()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    plan = sol.solve_plan(n, n_obs, retry=retry, has_x_init=x0 is not None, n_cu=ncu, tables_available=True)
    return _kernel_nodes(torch, d), plan


CASES = {
    "retry0": dict(retry=0),
    "retry1": dict(retry=1),
    "retry3": dict(retry=3),
    "das_fused_0": dict(retry=1, knobs=(("das_fused", 0),)),
    "prescreen": dict(retry=1, prescreen=True),
    "mixed": dict(retry=1, desc=dict(precision="mixed")),
    "force_generic_retry3": dict(retry=3, knobs=(("force_generic", 1),)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_a_captured_c1_call_launches_what_its_plan_says(api, torch_cuda, case):
    torch = torch_cuda
    c = CASES[case]
    desc, n, n_obs, arrays, x0 = _c1(api)
    kw = dict(precision=api.PRECISION_MIXED) if c.get("desc") else {}
    sol = api.Solver(api.make_desc(**desc, **kw))
    for k, v in c.get("knobs", ()):
        sol.set_knob(k, v)
    if c.get("prescreen"):
        sol.set_prescreen(api.PRESCREEN_ON)
    nodes, plan = _captured_and_planned(api, torch, sol, n, n_obs, arrays, x0, c["retry"])
    kinds = [p["kind"] for p in plan["passes"]]
    print(case, nodes, kinds)
    assert nodes == _expected(plan), (case, nodes, kinds)
    # what each case is here for
    assert ("fused" in kinds) == (case in ("retry0", "retry1", "retry3")), kinds
    assert ("prescreen" in kinds) == (case == "prescreen"), kinds
    if case == "force_generic_retry3":
        assert kinds == ["phase", "generic", "generic", "generic"], kinds


@pytest.mark.gpu
def test_a_batch_of_one_more_than_the_cus_launches_what_its_plan_says(api, torch_cuda):
    torch = torch_cuda
    desc, n, n_obs, arrays, x0 = _c1(api)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    reps = -(-(ncu + 1) // n)
    keep = ncu + 1  # (the first CUs + 1 instances of the repeated batch)
    hdr, rows, sfc = (np.concatenate([a] * reps) for a in (arrays[0], arrays[1], arrays[3]))
    offs = np.concatenate([arrays[2][:-1] + r * arrays[2][-1] for r in range(reps)] + [[reps * arrays[2][-1]]]).astype(np.uint64)
    sol = api.Solver(api.make_desc(**desc))
    nodes, plan = _captured_and_planned(api, torch, sol, keep, n_obs, (hdr, rows, offs, sfc), np.concatenate([x0] * reps)[:keep], 1)
    kinds = [p["kind"] for p in plan["passes"]]
    print(nodes, kinds)
    assert "fused" not in kinds and kinds[0] == "phase" and plan["passes"][0]["kmax"] == 20, plan
    assert nodes == _expected(plan), (nodes, kinds)


@pytest.mark.gpu
def test_beyond_the_carve_the_plan_says_fused_and_the_call_launches_the_fallback(api, torch_cuda):
    """The budgets of tests/test_das_fused_budgets.py that lie beyond the fused unit's compiled carve: the planner knows only the host-side
    eligibility, the launcher refuses, and the phase and the first pass run as two launches."""
    torch = torch_cuda
    desc, n, n_obs, arrays, x0 = _batch(api, "c3s")  # (M = 10 in 3-D: the carve holds 20 active rows; 32 is refused)
    sol = api.Solver(api.make_desc(**desc))
    sol.set_knob("das_kmax", 32)
    nodes, plan = _captured_and_planned(api, torch, sol, n, n_obs, arrays, x0, 1)
    kinds = [p["kind"] for p in plan["passes"]]
    print(nodes, kinds)
    assert kinds[0] == "fused" and plan["passes"][0]["kmax"] == 32, plan
    assert nodes == _expected(plan, fused_accepts=False), (nodes, kinds)
