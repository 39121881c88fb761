"""The dual active-set phase and the first interior-point pass in ONE launch (csrc/lscqp_fused.hip) against the two launches it replaces.

A batch of at most one instance per CU whose chosen fp64 instance has a fused form runs das_pdip_kernel: the workgroup that hands its
instance over solves it itself, with the pass's own class.  Everything here is bit for bit: the handle's `das_fused` knob on and off, same
batch, same start -- x, obj, status and info.  Plus the launch count of a captured call (one kernel fused; two beyond the CU count and with
the knob off; one, the phase alone, for LSCQP_ACTIVE_SET_ONLY) and a torch.cuda.graph replay of the fused call."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H


def _batch(api, key):
    import bench
    from lsc_dr_planner_amd import synth

    cfg = bench.CONFIGS[key]
    N, M, dim = cfg["agents"], cfg["segments"], cfg["dim"]
    sw, sol, build, (hdr, rows, off, sfc) = bench.make_batch(
        api, synth, lambda s: api.Solver(api.make_desc(M=M, dim=dim, world_min=s.world_min, world_max=s.world_max)), N, M, dim, cfg["obs"],
        seed=cfg["seed"], style=cfg["style"], warm_steps=cfg.get("warm_steps", 3))
    if cfg.get("infeasible_frac"):
        rows, _ = bench.make_infeasible(api, rows, hdr, sw.n_obs, M, cfg["infeasible_frac"], cfg["seed"] + 17)
    desc = dict(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max)
    return desc, N, sw.n_obs, (hdr, rows, off, sfc), api.x_init_from_swarm(build, dim)


class _Dev:
    """One batch on the device and the buffers of its results."""

    def __init__(self, torch, sol, n, n_obs, arrays, x0):
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        self.torch, self.sol, self.n, self.n_obs = torch, sol, n, n_obs
        self.inp = [up(a) for a in arrays]
        self.x0 = None if x0 is None else torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)).to(dev)
        self.x = torch.zeros(n * sol.nv, dtype=torch.float64, device=dev)
        self.obj = torch.zeros(n, dtype=torch.float64, device=dev)
        self.st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.info = torch.zeros(n * np.dtype(_info_dtype()).itemsize, dtype=torch.uint8, device=dev)

    def solve(self):
        self.sol.solve_device(self.n, self.n_obs, *self.inp, self.x, self.obj, self.st, self.info, d_x_init=self.x0)

    def result(self):
        self.torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (self.x, self.obj, self.st, self.info)]

    def clear(self):
        self.x.zero_(), self.obj.zero_(), self.st.fill_(-1), self.info.zero_()


def _info_dtype():
    from lsc_dr_planner_amd import api

    return api.INFO_DTYPE


def _solve(api, torch, desc, n, n_obs, arrays, x0, fused, knobs=(), **kw):
    sol = api.Solver(api.make_desc(**desc, **kw))
    sol.set_knob("das_fused", 1 if fused else 0)
    for k, v in knobs:
        sol.set_knob(k, v)
    d = _Dev(torch, sol, n, n_obs, arrays, x0)
    d.solve()
    return d.result()


def _same(a, b):
    return all(u.shape == v.shape and np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)) for u, v in zip(a, b))


def _hip():
    """The HIP runtime this process (torch and the library) already uses."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64.so" in path:
            return C.CDLL(path)
    raise RuntimeError("libamdhip64 is not loaded")


def _kernel_nodes(torch, d):
    """Kernel launches of one call of d, captured into a HIP graph (never launched)."""
    hip = _hip()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
        d.solve()
        g = C.c_void_p()
        assert hip.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(g)) == 0
    try:
        cnt = C.c_size_t(0)
        assert hip.hipGraphGetNodes(g, None, C.byref(cnt)) == 0
        nodes = (C.c_void_p * cnt.value)()
        assert hip.hipGraphGetNodes(g, nodes, C.byref(cnt)) == 0
        kinds = []
        for nd in nodes:
            t = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(nd), C.byref(t)) == 0
            kinds.append(t.value)
    finally:
        hip.hipGraphDestroy(g)
    return sum(1 for t in kinds if t == 0)  # hipGraphNodeTypeKernel


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
