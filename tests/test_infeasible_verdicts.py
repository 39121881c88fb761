"""The solver's INFEASIBLE verdicts against the exact feasibility referee (tests/feasibility.py), on every path that can give one.

Families A (near-antiparallel pairs), B (graded slabs) and C (empty and zero-width corridor intervals) on the c1 shape (M = 5, 3-D), the c0
shape (M = 10, 2-D), M = 9 in 3-D, and M = 12 in 3-D, which has no compiled instance: there paths a, b, c and e end in the run-time-shaped
kernel (csrc/lscqp_generic.hip), whose early-stop rules are an implementation of their own.  Paths:
  a  the default small batch through the device entry (at most one instance per CU: the fused launch);
  b  the same instances replicated past the CU count (two launches, the large-batch phase budget);
  c  knob das_fused = 0;
  d  LSCQP_ACTIVE_SET_ONLY (the phase alone: a verdict or a hand-over);
  e  knob active_set_off = 1 through the device entry (the interior-point kernel alone);
  g  knobs force_generic = 1 and active_set_off = 1 through the device entry: the run-time-shaped kernel alone, its own verdict on every shape
     (held to rules 1 - 4 like path e).
Rules: 1. FEASIBLE is never INFEASIBLE.  2. INFEASIBLE is never OPTIMAL.  3. t_hi <= -1e-4 is OPTIMAL on every path but d, at polish_primal's
point to 1e-8 m (the phase's answer) or 1e-6 m (the interior-point kernel's).  4. An empty corridor interval is INFEASIBLE with its overlap
(bmin - bmax) in res_primal.  5. Outside GREY, the phase on (a) and off (e) agree on OPTIMAL or not -- except that a FEASIBLE instance
with less than 1e-5 m of margin may end ITER_LIMIT with the phase off (the interior-point kernel's iteration budget, not a verdict)."""
from collections import Counter

import numpy as np
import pytest

from tests import feasibility as F
from tests import helpers as H

PATHS = ("a", "b", "c", "d", "e", "g")


def _device(torch, sol, arrays, n_obs):
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    n = len(arrays[0])
    x = torch.zeros(n * sol.nv, dtype=torch.float64, device=dev)
    obj = torch.zeros(n, dtype=torch.float64, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    info = torch.zeros(n * np.dtype(api_info()).itemsize, dtype=torch.uint8, device=dev)
    sol.solve_device(n, n_obs, *[up(a) for a in arrays], x, obj, st, info)
    torch.cuda.synchronize()
    return dict(x=x.cpu().numpy().reshape(n, sol.nv), status=st.cpu().numpy(), info=info.cpu().numpy().view(api_info()))


def api_info():
    from lsc_dr_planner_amd import api

    return api.INFO_DTYPE


def _assert_run_time_shaped(api, sol, n, n_obs):
    """The handle's next launch of n instances goes to the run-time-shaped kernel: lscqp_instance_work selects through the launch's own
    find_instance() call and switches, and answers ERR_UNSUPPORTED exactly when that finds no compiled instance."""
    with pytest.raises(api.LscqpError) as e:
        sol.instance_work(n, n_obs)
    assert e.value.code == api.ERR_UNSUPPORTED and "run-time-shaped kernel carries no instruction counts" in str(e.value), e.value


def _run_paths(api, torch, g, ncu):
    """Every path on the group's instances, in chunks of at most ncu / 2 instances (path a stays a small batch)."""
    out = {p: [] for p in PATHS}
    chunk = max(1, min(128, ncu // 2))
    for c0 in range(0, len(g.insts), chunk):
        part = g.insts[c0:c0 + chunk]
        arrays = F.to_batch(api, part, g.n_obs, g.M)
        n = len(part)
        sol = api.Solver(g.desc(api))
        out["a"].append(_device(torch, sol, arrays, g.n_obs))
        reps = ncu // n + 2  # past the CU count
        hdr, rows, off, sfc = F.to_batch(api, part * reps, g.n_obs, g.M)
        R = sol.solve_host(hdr, rows, off, sfc)
        out["b"].append({k: R[k][:n] for k in ("x", "status", "info")})
        for r in range(1, reps):  # every copy answers alike
            assert np.array_equal(R["status"][r * n:(r + 1) * n], R["status"][:n])
        sol.set_knob("das_fused", 0)
        out["c"].append(sol.solve_host(*arrays))
        sol.set_knob("das_fused", 1)
        only = api.Solver(g.desc(api, active_set=api.ACTIVE_SET_ONLY))
        out["d"].append(only.solve_host(*arrays))
        sol.set_knob("active_set_off", 1)
        out["e"].append(_device(torch, sol, arrays, g.n_obs))
        sol.set_knob("active_set_off", 0)
        gen = api.Solver(g.desc(api))
        if g.M > 10:  # no compiled instance: what paths a, b, c and e ran behind the phase was the run-time-shaped kernel already
            _assert_run_time_shaped(api, gen, n, g.n_obs)
        gen.set_knob("force_generic", 1)
        gen.set_knob("active_set_off", 1)
        _assert_run_time_shaped(api, gen, n, g.n_obs)
        out["g"].append(_device(torch, gen, arrays, g.n_obs))
    return {p: {k: np.concatenate([r[k] for r in out[p]]) for k in ("x", "status", "info")} for p in PATHS}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(F.SHAPES))
def test_infeasible_verdicts_against_the_referee(api, oracle, torch_cuda, shape):
    torch = torch_cuda
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    groups = F.build_groups(api, oracle, shape)
    insts = [i for g in groups for i in g.insts]
    counts = F.label_counts(insts)
    # non-vacuity: the sweep still reaches the places it exists for
    for fam in ("A", "B", "C"):
        assert counts[(fam, F.FEASIBLE)] > 0 and counts[(fam, F.INFEASIBLE)] > 0, sorted(counts.items())
    window = sum(i.kind3_window and i.label == F.FEASIBLE for i in insts)
    assert window >= 10, (window, sorted(counts.items()))

    fails = []
    table = Counter()
    for g in groups:
        R = _run_paths(api, torch, g, ncu)
        cls = g.oracle_class(oracle)
        for q, i in enumerate(g.insts):
            st = {p: int(R[p]["status"][q]) for p in PATHS}
            info = {p: R[p]["info"][q] for p in PATHS}
            for p in PATHS:
                table[(p, i.label, st[p])] += 1

            def fail(rule, p, extra=""):
                fails.append("rule %s path %s %s/%s %s %r: status %d %s" % (rule, p, g.name, i.family, i.params, i.verdict, st.get(p, st["a"]), extra))

            for p in PATHS:
                if i.label == F.FEASIBLE and st[p] == api.STATUS_INFEASIBLE:
                    fail(1, p, "res_primal %.3g flags %d" % (info[p]["res_primal"], info[p]["flags"]))
                if i.label == F.INFEASIBLE and st[p] == api.STATUS_OPTIMAL:
                    fail(2, p)
            if i.verdict.t_hi <= -1e-4:
                ag, lsc, sfc = F.oracle_inputs(oracle, i.hdr, i.rows, i.sfc)
                xr, ok = H.polish_primal(oracle, cls, ag, lsc, sfc)
                for p in ("a", "b", "c", "e", "g"):
                    if st[p] != api.STATUS_OPTIMAL:
                        fail(3, p)
                        continue
                    tol = 1e-8 if info[p]["flags"] & api.INFO_ACTIVE_SET else 1e-6
                    err = np.abs(R[p]["x"][q] - xr).max()
                    if ok and err > tol:
                        fail(3, p, "|x - x*| = %.3g > %.0e" % (err, tol))
                if st["d"] not in (api.STATUS_OPTIMAL, api.STATUS_ITER_LIMIT):
                    fail(3, "d")
            if i.family == "C" and i.params["gap"] > 0:
                for p in PATHS:
                    res = float(info[p]["res_primal"])
                    if st[p] != api.STATUS_INFEASIBLE or abs(res - i.params["gap"]) > 1e-14 + 1e-9 * i.params["gap"]:
                        fail(4, p, "res_primal %.6g, overlap %.6g" % (res, i.params["gap"]))
            if i.label != F.GREY and (st["a"] == api.STATUS_OPTIMAL) != (st["e"] == api.STATUS_OPTIMAL):
                # (known limit, counted in the table: with less than 1e-5 m of margin the interior-point kernel alone can run out of
                # iterations on a corridor face tilted against a row -- ITER_LIMIT, a failure, never a verdict; rule 1 holds it to that)
                if not (i.label == F.FEASIBLE and i.verdict.t_hi > -1e-5 and st["e"] == api.STATUS_ITER_LIMIT):
                    fail(5, "a/e", "phase off: status %d" % st["e"])
    if fails:
        lines = ["%s %-10s status %d: %d" % (p, lab, s, n) for (p, lab, s), n in sorted(table.items())]
        pytest.fail("%d violations on %s\n%s\ncounts (path, label, status):\n%s" % (len(fails), shape, "\n".join(fails[:40]), "\n".join(lines)))
