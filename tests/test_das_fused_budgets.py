"""Run-time budgets inside the fused kernel's compile-time LDS carve (csrc/lscqp_fused.hip, FusedCarve).

The fused phase lays out its LDS from its instance's maxima (active rows KMAX, the table copy, the staged rows of MAX_OBS obstacles); the
budgets of a launch -- das_kmax, das_steps, das_cache, das_stage -- stay run-time values.  A budget at or below the carve is served by the
fused form (one launch) and gives the bits of the two launches it replaces; a request beyond the carve is refused by the fused launcher
and runs as two launches, with the same bits.

What the bits can and cannot show: das_kmax and das_steps change which instances the phase hands over, so a fused form that ignored them
would differ.  das_cache = 0 and das_stage = 0 only move where the table and the rows are read from -- the same values -- so those cases
show that the fused form still serves the launch and stays in bounds, not that it honours the budget.  Hand-overs and their reason codes
are not observable here: the interior-point pass overwrites the record of every instance the phase hands over."""
import pytest

from tests.test_das_fused import _batch, _Dev, _kernel_nodes, _same


def _run(api, torch, desc, n, n_obs, arrays, x0, fused, knobs):
    """Results of one call, and the kernel launches of the same call captured into a graph."""
    sol = api.Solver(api.make_desc(**desc))
    sol.set_knob("das_fused", 1 if fused else 0)
    for k, v in knobs:
        sol.set_knob(k, v)
    d = _Dev(torch, sol, n, n_obs, arrays, x0)
    d.solve()  # (eager first: the class's tables reach the device before a capture)
    r = d.result()
    d.clear()
    return r, _kernel_nodes(torch, d)


BUDGETS = {
    "kmax4": (("das_kmax", 4),),
    "kmax8_steps2": (("das_kmax", 8), ("das_steps", 2)),
    "kmax1_steps1": (("das_kmax", 1), ("das_steps", 1)),
    "no_table_copy": (("das_cache", 0),),
    "no_staged_rows": (("das_stage", 0),),
}


@pytest.mark.gpu
@pytest.mark.parametrize("budget", sorted(BUDGETS))
@pytest.mark.parametrize("key", ["c1", "c0_loaded", "c1_loaded", "c1_infeasible_1pct"])
def test_budgets_below_the_carve_run_fused_and_bit_identical(api, torch_cuda, key, budget):
    torch = torch_cuda
    desc, n, n_obs, arrays, x0 = _batch(api, key)
    a, ka = _run(api, torch, desc, n, n_obs, arrays, x0, True, BUDGETS[budget])
    b, kb = _run(api, torch, desc, n, n_obs, arrays, x0, False, BUDGETS[budget])
    assert ka == 1 and kb == 2, (key, budget, ka, kb)
    assert _same(a, b), (key, budget)


@pytest.mark.gpu
def test_budget_beyond_the_carve_runs_two_launches(api, torch_cuda):
    # the 128-QP shard of configs[3] (M = 10 in 3-D): its carve holds 20 active rows beside the staged rows and the table; 32 is refused
    torch = torch_cuda
    desc, n, n_obs, arrays, x0 = _batch(api, "c3s")
    knobs = (("das_kmax", 32),)
    a, ka = _run(api, torch, desc, n, n_obs, arrays, x0, True, knobs)
    b, kb = _run(api, torch, desc, n, n_obs, arrays, x0, False, knobs)
    assert ka == 2 and kb == 2, (ka, kb)
    assert _same(a, b)
    c, kc = _run(api, torch, desc, n, n_obs, arrays, x0, True, (("das_kmax", 20),))
    assert kc == 1
