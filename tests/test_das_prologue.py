"""The prologue of the dual active-set phase (csrc/lscqp_das_body.inc up to its first pass): the kernel-argument block, the one wave of
requests with its clamped addresses, the rows asked for ahead of the header's trip through LDS, and the one-barrier verdict on an empty
interval -- on the inputs at which an address, a count or a flag of that code can go wrong.

Small batches (at most 8 instances) of the two smallest fused shapes, M5 in 3-D and M10 in 2-D, each through four forms of the kernel: the
fused launch (the rescheduled prologue of the phase's latency text, LSCQP_DAS_FORM LSCQP_DAS_LATENCY: both shapes' fused forms run it; one
test asserts that this form IS one launch), the two launches with 256 threads per instance, and the one- and two-wavefront forms
(das_threads 64 / 128), which run the throughput text: every value read where it is used.  Every form
must return the same bytes in x, obj, status and info; every instance the batch expects OPTIMAL is finished by the phase and held to the
polished CPU oracle at the bars of tests/test_das_families_gpu.py (x 1e-8 m, objective 1e-8 relative); every other instance to the status
the batch names.  Nothing is left out of the comparison.

Covered elsewhere and therefore not here: terminal_segments = 1 / between / M given in the header WITH active-set steps, in every form
including 16-byte rows (tests/test_das_families_gpu.py on das_cases.terminal_cases); a bogus obstacle count far beyond the capacity
(tests/test_active_set.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import das_cases as DC
from tests import helpers as H

pytestmark = pytest.mark.gpu

X_TOL, OBJ_TOL = 1e-8, 1e-8  # tests/test_das_families_gpu.py
SHAPES = [(5, 3), (10, 2)]
SHAPE_IDS = ["M5d3", "M10d2"]
FORMS = [("fused", dict(das_fused=1)), ("two launches", dict(das_fused=0)), ("one wavefront", dict(das_fused=0, das_threads=64)),
         ("two wavefronts", dict(das_fused=0, das_threads=128))]
OPTIMAL, CAPACITY, EMPTY = "optimal", "capacity", "empty interval"


class Batch:
    """ABI arrays of one call + what every instance must come back as + the oracle's inputs of the instances expected OPTIMAL"""

    def __init__(self, desc, ocls, M, hdr, rows, off, sfc, n_obs_max, expect, agents, lscs, boxes, order=None):
        self.desc, self.ocls, self.M, self.hdr, self.rows, self.off, self.sfc = desc, ocls, M, hdr, rows, off, sfc
        self.n_obs_max, self.expect, self.agents, self.lscs, self.boxes, self.order = n_obs_max, expect, agents, lscs, boxes, order
        self.ref = None  # (the oracle's answers: computed once)


def _relayout(api, hdr, rows, off, M, seed):
    """the instances' rows at different strides, one gap of 37 rows, everything between them NaN (a row read from there poisons its instance)"""
    rng = np.random.RandomState(seed)
    n = len(hdr)
    cnt = [int(off[q + 1] - off[q]) for q in range(n)]
    pad = [int(rng.randint(1, 9)) for _ in range(n)]
    pad[n // 2] = 37
    new_off = np.zeros(n + 1, np.uint64)
    at = 5
    for q in range(n):
        new_off[q] = at
        at += cnt[q] + pad[q]
    new_off[n] = at
    out = np.zeros(at, api.ROW_DTYPE)
    for f in ("nx", "ny", "nz", "b"):
        out[f] = np.nan
    for q in range(n):
        out[int(new_off[q]):int(new_off[q]) + cnt[q]] = rows[int(off[q]):int(off[q + 1])]
    assert n < 4 or len({int(new_off[q + 1] - new_off[q]) for q in range(n)}) > 2
    return out, new_off


def _swarm_inputs(api, O, M, dim, n_obs, seed):
    from lsc_dr_planner_amd import synth

    sw = synth.Swarm(max(24, n_obs + 4), M=M, dim=dim, n_obs=n_obs, seed=seed)
    assert sw.n_obs == n_obs
    b = sw.build()
    desc = lambda **kw: api.make_desc(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max, **kw)  # noqa: E731
    ocls = lambda **kw: O.make_class(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max, **kw)  # noqa: E731

    def agent(q, k):
        return O.make_agent(p0=b["p0"][q], v0=b["v0"][q], a0=b["a0"][q], goal=b["goal"][q], next_waypoint=b["next_waypoint"][q],
                            vmax=[sw.vmax] * 3, amax=[sw.amax] * 3, radius=sw.radius, nominal_velocity=sw.nominal_velocity, n_obs=k)

    def lsc(q, k):
        return np.ascontiguousarray(b["lsc"][q][:k]) if k else None

    def box(q):
        s = np.zeros(M, O.BOX_DTYPE)
        s["bmin"], s["bmax"] = b["sfc"]["bmin"][q], b["sfc"]["bmax"][q]
        return s

    return sw, desc, ocls, agent, lsc, box


def capacity_of(api, M, dim):
    """the obstacle capacity of the kernel instance a small launch of this shape selects (the phase's `cap`)"""
    sol = api.Solver(api.make_desc(M=M, dim=dim))
    cap = sol.instance_work(8, 1)["max_obstacles"]
    assert sol.instance_work(8, cap)["max_obstacles"] == cap
    return cap


def mixed_counts(api, O, M, dim, cap, with_rows=True, use_sfc=True, order=None, n=8):
    """n_obs = 0, 1, cap and cap + 1 next to ordinary neighbours; rows at different strides with a gap (with_rows False: nobody has a row and
    the call passes no row pointers)"""
    sw, desc, ocls, agent, lsc, box = _swarm_inputs(api, O, M, dim, cap, seed=11)
    counts = ([cap, 0, 1, cap + 1, 3, cap, 5, 2] if with_rows else [0] * 8)[:n]
    agents = [agent(q, min(k, cap)) for q, k in enumerate(counts)]
    lscs = [lsc(q, min(k, cap)) for q, k in enumerate(counts)]
    boxes = [box(q) for q in range(n)]
    oc = ocls(use_sfc=use_sfc)
    hdr, rows, off, sfc = H.abi_batch(api, O, oc, agents, lscs, boxes, M)
    expect = [CAPACITY if k > cap else OPTIMAL for k in counts]
    if with_rows:
        rows, off = _relayout(api, hdr, rows, off, M, seed=5)
        hdr["n_obs"] = counts  # (the refused instance claims one obstacle more than it has rows: none of them may be read)
    else:
        rows = off = None
    return Batch(desc(use_sfc=use_sfc), oc, M, hdr, rows, off, sfc if use_sfc else None, cap if with_rows else 0, expect, agents, lscs,
                 boxes if use_sfc else [None] * n, order=order)


def terminal_batch(api, O, M, dim):
    """terminal_segments GIVEN as 1, M and M + 3 (clamped to M), and LEFT to the kernel (0) with a flight time beyond the horizon (the rule
    of src/traj_optimizer.cpp:530-538 yields less than 1: 1) and with none to speak of (it yields M)"""
    spec = DC.spec_of(M, dim, "lsc")
    oc = DC.oracle_class(O, spec)
    d = float(np.hypot(1.0, 0.1))
    slow, fast = d / ((M + 2) * DC.DT), 1e12
    assert (M * DC.DT - d / slow + 1e-9) / DC.DT < 1 and int((M * DC.DT - d / fast + 1e-9) / DC.DT) == M
    agents, given = [], []
    for vn, ts in ((slow, 1), (fast, M), (fast, M + 3), (slow, 0), (fast, 0)):
        agents.append(O.make_agent(**dict(DC.LOOSE, **DC._hop(spec, 0, 1.0, vn=vn))))
        given.append(ts)
        assert O.terminal_segments(oc, agents[-1]) == (1 if vn == slow else M)
    boxes = [DC.wide_box(O, spec) for _ in agents]
    hdr, rows, off, sfc = H.abi_batch(api, O, oc, agents, [None] * len(agents), boxes, M)
    hdr["terminal_segments"] = given
    return Batch(DC.abi_desc(api, spec), oc, M, hdr, None, None, sfc, 0, [OPTIMAL] * len(agents), agents, [None] * len(agents), boxes)


def empty_interval_batch(api, O, M, dim):
    """one instance whose corridor box of the last segment lies 1 m beyond the world box on axis 0, among feasible ones"""
    spec = DC.spec_of(M, dim, "lsc")
    oc = DC.oracle_class(O, spec)
    agents = [O.make_agent(**dict(DC.LOOSE, **DC._hop(spec, k % dim, s))) for k, s in ((0, 1.0), (1, -1.0), (0, -1.0), (1, 1.0))]
    boxes = [DC.wide_box(O, spec) for _ in agents]
    bad = 2
    boxes[bad]["bmin"][M - 1][0] = spec["world_max"][0] + 1.0
    boxes[bad]["bmax"][M - 1][0] = spec["world_max"][0] + 2.0
    hdr, rows, off, sfc = H.abi_batch(api, O, oc, agents, [None] * len(agents), boxes, M)
    expect = [EMPTY if q == bad else OPTIMAL for q in range(len(agents))]
    b = Batch(DC.abi_desc(api, spec), oc, M, hdr, None, None, sfc, 0, expect, agents, [None] * len(agents), boxes)
    # lo - hi of the kernel's intervals on axis 0 of the last segment, largest: control points 3 and 4 (world face against the box), and the
    # last one, which the communication rows narrow as well (src/traj_optimizer.cpp:482-497)
    a = agents[bad]
    p0, wp = float(a["p0"][0]), float(a["next_waypoint"][0]) - float(a["p0"][0])
    rho_pair, rho_wp = 0.5 * DC.COMM_RANGE - float(a["radius"]), 0.5 * DC.COMM_RANGE - 1e-5
    lo, hi = spec["world_max"][0] + 1.0 - p0, spec["world_max"][0] - p0
    b.overlap = max(lo - hi, max(lo, max(-rho_pair, wp - rho_wp)) - min(hi, min(rho_pair, wp + rho_wp)))
    return b


def rsfc_batch(api, O, M, dim):
    """PLANNER_RSFC: z of segment 0 is bounded by +-100 instead of the world box -- the hump above the ceiling stays"""
    assert dim == 3
    spec = DC.spec_of(M, dim, "lsc")
    rs = dict(spec, planner="rsfc")
    relaxed = [c for c in DC.rsfc_cases(O, spec) if c.name == "rsfc_ceiling_relaxed"]
    assert len(relaxed) == 1
    oc = DC.oracle_class(O, rs)
    agents = [relaxed[0].agent, O.make_agent(**dict(DC.LOOSE, **DC._hop(rs, 2, 1.0))), O.make_agent(**dict(DC.LOOSE, **DC._hop(rs, 0, -1.0)))]
    boxes = [DC.wide_box(O, rs) for _ in agents]
    hdr, rows, off, sfc = H.abi_batch(api, O, oc, agents, [None] * len(agents), boxes, M)
    b = Batch(DC.abi_desc(api, rs), oc, M, hdr, None, None, sfc, 0, [OPTIMAL] * len(agents), agents, [None] * len(agents), boxes)
    b.above = relaxed[0].expect["above"]
    return b


_BATCHES = {}


def batch(name, make, *args, **kw):
    if name not in _BATCHES:
        _BATCHES[name] = make(*args, **kw)
    return _BATCHES[name]


def _device_call(api, torch, b, knobs):
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    sol = api.Solver(b.desc)
    for k, v in knobs.items():
        sol.set_knob(k, v)
    n = len(b.hdr)
    d_x = torch.zeros(n * sol.nv, dtype=torch.float64, device=dev)
    d_obj = torch.zeros(n, dtype=torch.float64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_info = torch.zeros(n * np.dtype(api.INFO_DTYPE).itemsize, dtype=torch.uint8, device=dev)
    d_order = None if b.order is None else torch.from_numpy(np.ascontiguousarray(b.order, dtype=np.int32)).to(dev)
    sol.solve_device(n, b.n_obs_max, up(b.hdr), up(b.rows), up(b.off), up(b.sfc), d_x, d_obj, d_st, d_info, d_order=d_order)
    torch.cuda.synchronize()
    return dict(x=d_x.cpu().numpy().reshape(n, -1), obj=d_obj.cpu().numpy(), status=d_st.cpu().numpy(), info=d_info.cpu().numpy().view(api.INFO_DTYPE))


def _kernel_launches(api, torch, b, knobs):
    """kernel launches of one call of the batch in this form: the call captured into a HIP graph that is never launched (as
    tests/test_das_fused.py counts them)"""
    hip = None
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line.split()[-1]:
            hip = C.CDLL(line.split()[-1])
            break
    assert hip is not None, "libamdhip64 is not loaded"
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    sol = api.Solver(b.desc)
    for k, v in knobs.items():
        sol.set_knob(k, v)
    n = len(b.hdr)
    d_x = torch.zeros(n * sol.nv, dtype=torch.float64, device=dev)
    d_obj = torch.zeros(n, dtype=torch.float64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_info = torch.zeros(n * np.dtype(api.INFO_DTYPE).itemsize, dtype=torch.uint8, device=dev)
    t = [up(a) for a in (b.hdr, b.rows, b.off, b.sfc)]
    call = lambda: sol.solve_device(n, b.n_obs_max, t[0], t[1], t[2], t[3], d_x, d_obj, d_st, d_info)  # noqa: E731
    call()  # (eager first: the class's tables reach the device before a capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
        call()
        g = C.c_void_p()
        assert hip.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(g)) == 0
    try:
        cnt = C.c_size_t(0)
        assert hip.hipGraphGetNodes(g, None, C.byref(cnt)) == 0
        nodes = (C.c_void_p * cnt.value)()
        assert hip.hipGraphGetNodes(g, nodes, C.byref(cnt)) == 0
        kernels = 0
        for nd in nodes:
            kind = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(nd), C.byref(kind)) == 0
            kernels += kind.value == 0  # hipGraphNodeTypeKernel
    finally:
        hip.hipGraphDestroy(g)
    return kernels


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)) for f in ("x", "obj", "status", "info"))


def every_form(api, O, torch, b):
    """the batch through every form: the same bytes, every instance what the batch expects, every OPTIMAL one at the oracle's optimum"""
    res = [(name, _device_call(api, torch, b, knobs)) for name, knobs in FORMS]
    G = res[0][1]
    for name, r in res[1:]:
        assert _same(r, G), (name, r["status"], G["status"], r["info"], G["info"])
    if b.ref is None:
        b.ref = {}
        for q, e in enumerate(b.expect):
            if e == OPTIMAL:
                r = O.solve(b.ocls, b.agents[q], b.lscs[q], b.boxes[q])
                assert r["status"] == 0, ("the oracle solves every feasible instance", q)
                b.ref[q] = (r["x"], DC.objective(O.assemble(b.ocls, b.agents[q], b.lscs[q], b.boxes[q]), r["x"]))
    info = G["info"]
    for q, e in enumerate(b.expect):
        if e == OPTIMAL:
            xr, fr = b.ref[q]
            assert G["status"][q] == api.STATUS_OPTIMAL and (info["flags"][q] & api.INFO_ACTIVE_SET), (q, G["status"][q], info[q])
            dx, dobj = np.abs(G["x"][q] - xr).max(), abs(G["obj"][q] - fr) / max(1.0, abs(fr))
            print("prologue| instance %d: %d steps, |dx| %.1e m, objective %.1e rel" % (q, info["iterations"][q], dx, dobj))
            assert dx <= X_TOL and dobj <= OBJ_TOL, (q, dx, dobj)
        elif e == CAPACITY:
            assert G["status"][q] == api.STATUS_CAPACITY, (q, G["status"][q])
        else:
            assert G["status"][q] == api.STATUS_INFEASIBLE and info["iterations"][q] == 0 and (info["flags"][q] & api.INFO_ACTIVE_SET), (q, G["status"][q], info[q])
    return G


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixed_obstacle_counts_at_uneven_row_offsets(api, oracle, torch_cuda, shape):
    M, dim = shape
    cap = capacity_of(api, M, dim)
    b = batch(("mixed",) + shape, mixed_counts, api, oracle, M, dim, cap)
    assert sorted(set(b.hdr["n_obs"])) == sorted({0, 1, 2, 3, 5, cap, cap + 1})
    G = every_form(api, oracle, torch_cuda, b)
    assert np.isfinite(G["x"]).all() and np.isfinite(G["obj"]).all()  # (nothing between the instances' rows was read)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_fused_form_is_one_launch_and_the_others_more(api, oracle, torch_cuda, shape):
    """what every_form calls "fused" is the fused kernel, with rows and without: otherwise it would be a second copy of "two launches" """
    M, dim = shape
    cap = capacity_of(api, M, dim)
    for b in (batch(("mixed",) + shape, mixed_counts, api, oracle, M, dim, cap),
              batch(("no rows",) + shape, mixed_counts, api, oracle, M, dim, cap, with_rows=False)):
        assert _kernel_launches(api, torch_cuda, b, FORMS[0][1]) == 1
        for name, knobs in FORMS[1:]:
            assert _kernel_launches(api, torch_cuda, b, knobs) > 1, name  # (the phase, then the interior-point pass)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_call_without_any_rows(api, oracle, torch_cuda, shape):
    M, dim = shape
    b = batch(("no rows",) + shape, mixed_counts, api, oracle, M, dim, capacity_of(api, M, dim), with_rows=False)
    assert b.rows is None and b.off is None and b.n_obs_max == 0
    every_form(api, oracle, torch_cuda, b)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_an_order_of_the_launch_and_a_launch_of_one(api, oracle, torch_cuda, shape):
    M, dim = shape
    cap = capacity_of(api, M, dim)
    plain = batch(("mixed",) + shape, mixed_counts, api, oracle, M, dim, cap)
    b = batch(("ordered",) + shape, mixed_counts, api, oracle, M, dim, cap, order=[5, 2, 7, 0, 3, 6, 1, 4])
    b.ref = plain.ref  # (the same instances)
    G = every_form(api, oracle, torch_cuda, b)
    assert _same(G, _device_call(api, torch_cuda, plain, FORMS[0][1]))  # results land at the instance's own index
    one = batch(("one",) + shape, mixed_counts, api, oracle, M, dim, cap, order=[0], n=1)
    every_form(api, oracle, torch_cuda, one)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_terminal_segments_given_clamped_and_computed(api, oracle, torch_cuda, shape):
    M, dim = shape
    b = batch(("terminal",) + shape, terminal_batch, api, oracle, M, dim)
    G = every_form(api, oracle, torch_cuda, b)
    # the clamped count is the given M's, the computed ones are the given ones': to the bit
    assert np.array_equal(G["x"][2], G["x"][1]) and np.array_equal(G["x"][3], G["x"][0]) and np.array_equal(G["x"][4], G["x"][1])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_an_empty_interval_among_feasible_instances(api, oracle, torch_cuda, shape):
    M, dim = shape
    b = batch(("empty",) + shape, empty_interval_batch, api, oracle, M, dim)
    G = every_form(api, oracle, torch_cuda, b)
    bad = b.expect.index(EMPTY)
    assert abs(G["info"]["res_primal"][bad] - b.overlap) <= 1e-12, (G["info"][bad], b.overlap)
    assert G["obj"][bad] == 0.0 and np.array_equal(G["x"][bad].reshape(dim, -1), np.repeat(b.hdr["p0"][bad][:dim, None], 6 * M, axis=1))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_class_without_corridor_boxes(api, oracle, torch_cuda, shape):
    M, dim = shape
    cap = capacity_of(api, M, dim)
    b = batch(("no sfc",) + shape, mixed_counts, api, oracle, M, dim, cap, use_sfc=False)
    assert b.sfc is None
    every_form(api, oracle, torch_cuda, b)


def test_the_rsfc_class_keeps_the_hump_above_the_ceiling(api, oracle, torch_cuda):
    M, dim = 5, 3  # (PLANNER_RSFC relaxes the z interval of segment 0: 3-D only)
    b = batch("rsfc", rsfc_batch, api, oracle, M, dim)
    G = every_form(api, oracle, torch_cuda, b)
    assert G["x"][0].reshape(dim, M, 6)[2, 0].max() > b.above
