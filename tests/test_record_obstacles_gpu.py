"""The obstacle record's kernel alone (include/lscqp.h, "the obstacle record"; csrc/lscrecord.hip: record_obstacles_kernel): stand-alone
records driven by lscqp_record_step_device with constructed headers -- no QP is solved -- and constructed lscqp_safety_obs arrays, against
the plain-Python restatement (tests/record_obstacles_reference.py) field for field.  WHERE the kernel wrote is checked against a sentinel
in the spare bytes around the two arrays and in the slots of a frozen mission."""
import ctypes as C

import numpy as np
import pytest

from tests import record_obstacles_cases as RC
from tests import record_obstacles_reference as ROR

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)  # both sides of a wavefront and of the 256-thread workgroup (a second trip of the stride)
# name -> (offsets or None, n_total, the mission that finishes at replan 1)
PARTITIONS = {"K1": (None, 257, 0), "K2": (np.array([0, 65, 65 + 257]), 65 + 257, 1), "K5": (np.concatenate([[0], np.cumsum(SIZES)]), sum(SIZES), 3)}
M, DIM, DT, Z = 5, 3, 0.25, 1.0
SENTINEL = 0xA5


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _offsets(off, n):
    return np.array([0, n]) if off is None else np.asarray(off)


def _record(api, off, n, S=2):
    sol = api.Solver(api.make_desc(M=M, dim=DIM, dt=DT))
    return sol, api.Record(sol, n, off, S, 0.1, 0.2, Z, goal_threshold=0.5)


def _inputs(api, rng, n, goals, near=None):
    """One replan's inputs of the record itself (tests/test_flight_log_gpu.py: _inputs); `near`: the agents that start AT their goals."""
    hdr = np.zeros(n, api.HEADER_DTYPE)
    hdr["p0"] = goals + rng.uniform(1.0, 2.0, (n, 3))
    if near is not None:
        hdr["p0"][near] = goals[near]
    hdr["n_obs"] = rng.integers(0, 6, n)
    saf = np.zeros(n, api.SAFETY_DTYPE)
    saf["safety_ratio"] = rng.uniform(1.0, 3.0, n)
    saf["closest_agent"] = rng.integers(0, n, n)
    ints = dict(status=rng.integers(0, 5, n), goal_status=rng.integers(0, 3, n), sfc_status=rng.integers(0, 2, n), valid=rng.integers(0, 2, n),
                in_range=rng.integers(0, 9, n))
    return dict(x=rng.uniform(-4, 4, (n, DIM * M * 6)), hdr=hdr, saf=saf, **{k: v.astype(np.int32) for k, v in ints.items()})


def _step(torch, rec, I, stream=None):
    d = {k: _dev(torch, v) for k, v in I.items()}
    rec.step_device(d["hdr"], d["x"], d["status"], d["goal_status"], d["sfc_status"], d["valid"], d["in_range"], d["saf"], None, stream=stream)
    return d


def _near(offsets, k, n):
    near = np.zeros(n, bool)
    near[offsets[k]:offsets[k + 1]] = True
    return near


def _layout(api, offsets):
    """Byte ranges of the raw side buffer: (missions at, agents at, size)."""
    K, n, G = len(offsets) - 1, int(offsets[-1]), api.OBSREC_SPARE
    m_at = G
    a_at = m_at + K * api.MISSION_OBSTACLE_RECORD_DTYPE.itemsize + G
    return m_at, a_at, a_at + n * api.AGENT_OBSTACLE_RECORD_DTYPE.itemsize + G


def _expected(api, offsets, missions, agents):
    return ROR.as_arrays(np, api.MISSION_OBSTACLE_RECORD_DTYPE, api.AGENT_OBSTACLE_RECORD_DTYPE, missions, agents)


def _fly(api, torch, rec, offsets, figures, finish, seed, d_fig, twin=None):
    """The replans `figures` into `rec` (and the same inputs into `twin`), mission finish[0] finishing at replan finish[1] through its
    headers.  The restatement is fed what the record itself said before each replan.  Returns (missions, agents) per replan, restated."""
    n = int(offsets[-1])
    rng = np.random.default_rng(seed)
    goals = rng.uniform(-4, 4, (n, 3))
    rec.reset(goals)
    if twin is not None:
        twin.reset(goals)
    missions, agents = ROR.cleared(offsets)
    out = []
    for r, fig in enumerate(figures):
        before, _ = rec.download()
        d_fig.copy_(_dev(torch, fig))
        I = _inputs(api, rng, n, goals, _near(offsets, finish[0], n) if r == finish[1] else None)
        _step(torch, rec, I)
        ROR.accumulate(missions, agents, offsets, RC.triples(fig), before["finished"], before["replans"])
        if twin is not None:
            _step(torch, twin, I)
            (ra, da), (rb, db) = rec.download(), twin.download()
            assert ra.tobytes() == rb.tobytes() and da.tobytes() == db.tobytes() and rec.points().tobytes() == twin.points().tobytes(), r
            assert rec.unfinished() == twin.unfinished()
        out.append(_expected(api, offsets, missions, agents))
    return out


@pytest.mark.parametrize("log", [False, True], ids=["no-log", "log"])
@pytest.mark.parametrize("part", list(PARTITIONS))
def test_random_flights_equal_the_restatement_and_only_live_slots_are_written(api, torch_cuda, part, log):
    """Four replans of figures drawn from eight values (ties at every size, +inf, NaN, 1.0 and the double below it); one mission finishes at
    replan 1.  After every replan the download equals the restatement, field for field.  The spare bytes around the two arrays are filled
    with a sentinel before the flight, and behind replan 1 so are the frozen mission's slot and its agents' entries: after the flight every
    one of those bytes still holds it and every other byte is the restatement's.  The record's own structs, distances and points equal a
    twin record's that has no obstacle figures (both with a flight log, or both without), byte for byte after every replan."""
    torch = torch_cuda
    off, n, fz = PARTITIONS[part]
    offsets = _offsets(off, n)
    K = len(offsets) - 1
    sol, rec = _record(api, off, n)
    sol2, twin = _record(api, off, n)
    if log:
        rec.set_log(3, 1)
        twin.set_log(3, 1)
    rng = np.random.default_rng(61)
    figures = [RC.random_figures(rng, n, api.SAFETY_OBS_DTYPE) for _ in range(4)]
    d_fig = _dev(torch, figures[0])
    rec.set_obstacle_figures(d_fig)
    raw = rec.obstacles_tensor()
    m_at, a_at, size = _layout(api, offsets)
    assert raw.numel() == size
    G, msz, asz = api.OBSREC_SPARE, api.MISSION_OBSTACLE_RECORD_DTYPE.itemsize, api.AGENT_OBSTACLE_RECORD_DTYPE.itemsize
    spare = np.zeros(size, bool)
    spare[:G] = spare[m_at + K * msz:a_at] = spare[-G:] = True
    raw[torch.from_numpy(spare).cuda()] = SENTINEL
    want = _fly(api, torch, rec, offsets, figures[:2], (fz, 1), 67, d_fig, twin)
    ms, ag = rec.obstacles()
    assert RC.same_structs(ms, want[1][0]) and RC.same_structs(ag, want[1][1])
    assert rec.download()[0]["finished"].tolist() == [int(k == fz) for k in range(K)]
    # the frozen mission's slots: a sentinel from here on
    held = spare.copy()
    held[m_at + fz * msz:m_at + (fz + 1) * msz] = True
    held[a_at + offsets[fz] * asz:a_at + offsets[fz + 1] * asz] = True
    raw[torch.from_numpy(held).cuda()] = SENTINEL
    torch.cuda.synchronize()
    missions, agents = ([dict(zip(a.dtype.names, row.tolist())) for row in a] for a in want[1])
    goals = np.random.default_rng(67).uniform(-4, 4, (n, 3))  # (the goals _fly gave the records: its generator's first draw)
    rng2 = np.random.default_rng(71)
    for r in (2, 3):  # (the records are not reset: the flight goes on)
        before, _ = rec.download()
        assert before["finished"][fz] == 1 and before["replans"][fz] == 2
        d_fig.copy_(_dev(torch, figures[r]))
        I = _inputs(api, rng2, n, goals)
        _step(torch, rec, I)
        _step(torch, twin, I)
        ROR.accumulate(missions, agents, offsets, RC.triples(figures[r]), before["finished"], before["replans"])
        assert rec.download()[0].tobytes() == twin.download()[0].tobytes() and rec.points().tobytes() == twin.points().tobytes(), r
    torch.cuda.synchronize()
    got = raw.cpu().numpy()
    ems, eag = _expected(api, offsets, missions, agents)
    full = np.full(size, SENTINEL, np.uint8)
    full[m_at:m_at + K * msz] = ems.view(np.uint8)
    full[a_at:a_at + n * asz] = eag.view(np.uint8)
    full[held] = SENTINEL
    assert (got[held] == SENTINEL).all()
    assert got.tobytes() == full.tobytes(), np.flatnonzero(got != full)[:8]
    if K > 1:
        live = [k for k in range(K) if k != fz]
        ms, _ = rec.obstacles()
        assert RC.same_structs(ms[live], ems[live]) and ems["compared"][live].min() > 0
    for r_, s_ in ((rec, sol), (twin, sol2)):
        r_.close()
        s_.close()


def test_the_hand_table_on_the_device(api, torch_cuda):
    """tests/record_obstacles_cases.py: hand_table through the kernel -- mission 1 finishing at replan 1 through its headers -- gives the
    structs written out there by construction, and the record's finished / replans words are the ones the table assumes."""
    torch = torch_cuda
    offsets, steps, missions, agents = RC.hand_table()
    offsets = np.array(offsets)
    n = int(offsets[-1])
    sol, rec = _record(api, offsets, n)
    figures = [RC.figures_of(rows, api.SAFETY_OBS_DTYPE) for rows, _, _ in steps]
    d_fig = _dev(torch, figures[0])
    rec.set_obstacle_figures(d_fig)
    rng = np.random.default_rng(73)
    goals = rng.uniform(-4, 4, (n, 3))
    rec.reset(goals)
    for r, (rows, finished, replans) in enumerate(steps):
        before, _ = rec.download()
        assert before["finished"].tolist() == finished and before["replans"].tolist() == replans, r
        d_fig.copy_(_dev(torch, figures[r]))
        _step(torch, rec, _inputs(api, rng, n, goals, _near(offsets, 1, n) if r == 1 else None))
    ms, ag = rec.obstacles()
    ems, eag = _expected(api, offsets, missions, agents)
    for f in ems.dtype.names:
        assert ms[f].tolist() == ems[f].tolist(), f
    for f in eag.dtype.names:
        assert ag[f].tolist() == eag[f].tolist(), f
    rec.close()
    sol.close()


def test_reset_clears_the_figures_and_the_same_flight_gives_them_again(api, torch_cuda):
    torch = torch_cuda
    off, n, fz = PARTITIONS["K5"]
    offsets = _offsets(off, n)
    sol, rec = _record(api, off, n)
    rng = np.random.default_rng(79)
    figures = [RC.random_figures(rng, n, api.SAFETY_OBS_DTYPE) for _ in range(3)]
    d_fig = _dev(torch, figures[0])
    rec.set_obstacle_figures(d_fig)
    cleared = _expected(api, offsets, *ROR.cleared(offsets))
    ms, ag = rec.obstacles()
    assert RC.same_structs(ms, cleared[0]) and RC.same_structs(ag, cleared[1])  # (cleared when it was attached)
    first = None
    for _ in range(2):
        want = _fly(api, torch, rec, offsets, figures, (fz, 1), 83, d_fig)
        ms, ag = rec.obstacles()
        assert RC.same_structs(ms, want[-1][0]) and RC.same_structs(ag, want[-1][1])
        assert not RC.same_structs(ms, cleared[0])
        first = first or (ms.tobytes(), ag.tobytes())
        assert (ms.tobytes(), ag.tobytes()) == first
        rec.reset(np.zeros((n, 3)))
        ms, ag = rec.obstacles()
        assert RC.same_structs(ms, cleared[0]) and RC.same_structs(ag, cleared[1])
    rec.close()
    sol.close()


def _kernel_launches(torch, call):
    """Kernel nodes of one call captured into a HIP graph that is never launched (tests/test_das_prologue.py counts them so)."""
    hip = None
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line.split()[-1]:
            hip = C.CDLL(line.split()[-1])
            break
    assert hip is not None, "libamdhip64 is not loaded"
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
        call(s)
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


def test_one_launch_more_and_removal_restores_the_count(api, torch_cuda):
    """A step of a plain record is one launch, with a log two; the obstacle figures add exactly one to either, and removing them gives the
    count back -- with the download and the raw pointer refused, the cause named.  A record that never had them refuses too."""
    torch = torch_cuda
    off, n, _ = PARTITIONS["K2"]
    sol, rec = _record(api, off, n)
    rng = np.random.default_rng(89)
    goals = rng.uniform(-4, 4, (n, 3))
    rec.reset(goals)
    d = {k: _dev(torch, v) for k, v in _inputs(api, rng, n, goals).items()}
    d_fig = _dev(torch, RC.random_figures(rng, n, api.SAFETY_OBS_DTYPE))
    torch.cuda.synchronize()

    def count():
        return _kernel_launches(torch, lambda s: rec.step_device(d["hdr"], d["x"], d["status"], d["goal_status"], d["sfc_status"], d["valid"], d["in_range"],
                                                                 d["saf"], None, stream=s))

    with pytest.raises(api.LscqpError, match="keeps no obstacle figures") as e:
        rec.obstacles()
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    assert count() == 1
    rec.set_obstacle_figures(d_fig)
    assert count() == 2
    rec.set_log(2)
    assert count() == 3
    rec.set_obstacle_figures(None)
    assert count() == 2
    for call in (rec.obstacles, rec.obstacles_tensor):
        with pytest.raises(api.LscqpError, match="keeps no obstacle figures"):
            call()
    rec.set_log(0)
    assert count() == 1
    assert rec.download()[0]["replans"].tolist() == [0, 0]  # (captured, never launched)
    rec.close()
    sol.close()
