"""One batch of bench.CONFIGS on the device, and the kernel launches of one solve call of it counted in a captured HIP graph: shared by the
modules that compare launches (test_das_fused*.py, test_das_families_gpu.py, test_solve_plan_gpu.py)."""
import ctypes as C

import numpy as np


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
        self.torch, self.sol, self.n, self.n_obs, self.retry = torch, sol, n, n_obs, 0
        self.inp = [up(a) for a in arrays]
        self.x0 = None if x0 is None else torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)).to(dev)
        self.x = torch.zeros(n * sol.nv, dtype=torch.float64, device=dev)
        self.obj = torch.zeros(n, dtype=torch.float64, device=dev)
        self.st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.info = torch.zeros(n * np.dtype(_info_dtype()).itemsize, dtype=torch.uint8, device=dev)

    def solve(self):
        self.sol.solve_device(self.n, self.n_obs, *self.inp, self.x, self.obj, self.st, self.info, d_x_init=self.x0, retry=self.retry)

    def result(self):
        self.torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (self.x, self.obj, self.st, self.info)]

    def clear(self):
        self.x.zero_(), self.obj.zero_(), self.st.fill_(-1), self.info.zero_()


def _info_dtype():
    from lsc_dr_planner_amd import api

    return api.INFO_DTYPE


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
