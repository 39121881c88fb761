"""The dual active-set phase and the first interior-point pass in ONE launch (csrc/lscqp_fused.hip) against the two launches it replaces.

A batch of at most one instance per CU whose chosen fp64 instance has a fused form runs das_pdip_kernel: the workgroup that hands its
instance over solves it itself, with the pass's own class.  Everything here is bit for bit: the handle's `das_fused` knob on and off, same
batch, same start -- x, obj, status and info.  Plus the launch count of a captured call (one kernel fused; two beyond the CU count and with
the knob off; one, the phase alone, for LSCQP_ACTIVE_SET_ONLY) and a torch.cuda.graph replay of the fused call."""
import numpy as np
import pytest

from tests import helpers as H
from tests.das_capture import _batch, _Dev, _kernel_nodes, _same  # noqa: F401  (other modules take them from here)


def _solve(api, torch, desc, n, n_obs, arrays, x0, fused, knobs=(), **kw):
    sol = api.Solver(api.make_desc(**desc, **kw))
    sol.set_knob("das_fused", 1 if fused else 0)
    for k, v in knobs:
        sol.set_knob(k, v)
    d = _Dev(torch, sol, n, n_obs, arrays, x0)
    d.solve()
    return d.result()


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["c0_loaded", "c1_loaded", "c1_infeasible_1pct", "c1", "c3s"])
def test_fused_equals_two_launches_bit_for_bit(api, torch_cuda, key):
    torch = torch_cuda
    desc, n, n_obs, arrays, x0 = _batch(api, key)
    a = _solve(api, torch, desc, n, n_obs, arrays, x0, fused=True)
    b = _solve(api, torch, desc, n, n_obs, arrays, x0, fused=False)
    assert _same(a, b), key
    st, info = a[2], a[3].view(api.INFO_DTYPE)
    if key != "c1_infeasible_1pct":
        assert (st == 0).all(), (key, st)
    if key == "c1_infeasible_1pct":  # proven infeasible inside the phase: nothing for the interior-point half
        assert ((st == api.STATUS_INFEASIBLE) & ((info["flags"] & api.INFO_ACTIVE_SET) != 0)).any(), st


@pytest.mark.gpu
def test_fused_equals_two_launches_when_most_instances_are_handed_over(api, torch_cuda):
    torch = torch_cuda
    desc, n, n_obs, arrays, x0 = _batch(api, "c1_loaded")
    knobs = (("das_kmax", 1), ("das_steps", 1))
    a = _solve(api, torch, desc, n, n_obs, arrays, x0, fused=True, knobs=knobs)
    b = _solve(api, torch, desc, n, n_obs, arrays, x0, fused=False, knobs=knobs)
    assert _same(a, b)
    info = a[3].view(api.INFO_DTYPE)
    assert ((info["flags"] & api.INFO_ACTIVE_SET) == 0).sum() >= 8, info["flags"]
    assert (a[2] == 0).all()


@pytest.mark.gpu
def test_fused_equals_two_launches_on_the_log_pipeline_fixture(api, oracle, torch_cuda):
    torch = torch_cuda
    g = H.load_golden("kat_log_pipeline")
    p, cases = g["params"], g["cases"]
    M = p["M"]
    cls = H.oracle_class(oracle, p, use_sfc=True)
    arrs = [H.pipeline_case_arrays(oracle, p, c) for c in cases]
    ags = [mk(c["goal"]) for (L, box, mk), c in zip(arrs, cases)]
    hdr, rows, off, sfc = H.abi_batch(api, oracle, cls, ags, [a[0] for a in arrs], [a[1] for a in arrs], M)
    for q, c in enumerate(cases):
        hdr["terminal_segments"][q] = oracle.terminal_segments(cls, arrs[q][2](c["goal"]))
    n, n_obs = len(hdr), int(hdr["n_obs"].max())
    res = []
    for fused in (True, False):
        s = api.Solver(H.abi_desc(api, p, use_sfc=True))
        s.set_knob("das_fused", 1 if fused else 0)
        d = _Dev(torch, s, n, n_obs, (hdr, rows, off, sfc), None)
        d.solve()
        res.append(d.result())
    assert _same(res[0], res[1])
    assert (res[0][2] == 0).all(), res[0][2]


@pytest.mark.gpu
def test_launch_count_fused_two_launches_and_active_set_only(api, torch_cuda):
    torch = torch_cuda
    desc, n, n_obs, arrays, x0 = _batch(api, "c1")

    def nodes(fused, n_, **kw):
        sol = api.Solver(api.make_desc(**desc, **kw))
        sol.set_knob("das_fused", 1 if fused else 0)
        d = _Dev(torch, sol, n_, n_obs, arrays, x0)
        d.solve()  # (eager first: the class's tables reach the device before a capture)
        r = d.result()
        d.clear()
        return _kernel_nodes(torch, d), r

    assert nodes(True, n)[0] == 1
    assert nodes(False, n)[0] == 2
    # a batch beyond the CU count keeps the phase and the pass as two launches
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    reps = -(-(ncu + 1) // n)
    big = [np.concatenate([a] * reps) for a in (arrays[0], arrays[1], arrays[3])]
    offs = np.concatenate([arrays[2][:-1] + r * arrays[2][-1] for r in range(reps)] + [[reps * arrays[2][-1]]]).astype(np.uint64)
    nb = n * reps
    sol = api.Solver(api.make_desc(**desc))
    d = _Dev(torch, sol, nb, n_obs, (big[0], big[1], offs, big[2]), np.concatenate([x0] * reps))
    d.solve()
    d.result()
    assert nb > ncu and _kernel_nodes(torch, d) == 2
    # LSCQP_ACTIVE_SET_ONLY: the phase alone, the same bits whatever the knob says
    k1, r1 = nodes(True, n, active_set=api.ACTIVE_SET_ONLY)
    k0, r0 = nodes(False, n, active_set=api.ACTIVE_SET_ONLY)
    assert k1 == 1 and k0 == 1 and _same(r1, r0)


@pytest.mark.gpu
def test_fused_call_replays_in_a_torch_cuda_graph(api, torch_cuda):
    torch = torch_cuda
    desc, n, n_obs, arrays, x0 = _batch(api, "c1_loaded")
    ref = _solve(api, torch, desc, n, n_obs, arrays, x0, fused=False)
    sol = api.Solver(api.make_desc(**desc))
    d = _Dev(torch, sol, n, n_obs, arrays, x0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d.solve()  # warm-up (tables on the device)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d.solve()
    for _ in range(2):
        d.clear()
        g.replay()
        assert _same(d.result(), ref)
