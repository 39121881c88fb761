"""lscqp_waypoints_wide_device, the many-workgroup form of the waypoint decision, against lscqp_waypoints_device (one workgroup) and the plain
Python restatement of the reference (tests/grid_reference.py).  Each case goes through all three and every comparison is exact equality of
the group, the desired node, the updated flag and the waypoint buffer.  Where a case breaks PIBT's precondition (two members of a group on
one waypoint node) the restatement is undefined and the two device entries are compared alone; the case says so."""
import numpy as np
import pytest

from tests import grid_reference as R
from tests import waypoint_cases as WC
from tests import waypoint_device as WD

pytestmark = pytest.mark.gpu
f32 = np.float32


def _step(torch, grid, wide, rng, s, d_field, d_init_d):
    return WD.decision_step(torch, grid, rng, s, d_field, d_init_d, wide=wide)


def _compare(torch, grid, G, rng, s, F, init_d, d_field, d_init_d, restatement=True):
    """wide == one workgroup == restatement; returns the wide entry's (group, desired, updated, waypoints)."""
    wide = _step(torch, grid, True, rng, s, d_field, d_init_d)
    one = _step(torch, grid, False, rng, s, d_field, d_init_d)
    for name, a, b in zip(("group", "desired", "updated", "waypoint"), wide, one):
        assert np.array_equal(a, b), (name, "wide != one workgroup", np.nonzero(np.asarray(a != b).reshape(len(a), -1).any(axis=1))[0][:10])
    if restatement:
        ref = R.waypoint_step(G, rng, s["positions"], None if s["plans"] is None else list(s["plans"]), s["current_goals"], s["waypoints"], F, init_d)
        for name, a, b in zip(("group", "desired", "updated", "waypoint"), wide, ref):
            assert np.array_equal(a, b), (name, "wide != restatement", np.nonzero(np.asarray(a != b).reshape(len(a), -1).any(axis=1))[0][:10])
    return wide


@pytest.mark.parametrize("name", sorted(WC.TOYS))
def test_wide_on_toy_cases(api, oracle, torch_cuda, name):
    import torch

    c = WC.toy_case(name)
    wmap, grid = WD.device_grid(api, c["world"])
    G = WC.reference_grid(oracle, c["world"])
    F, init_d = R.mission_fields(G, c["starts"], c["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, c["starts"], c["goals"])
    if c["init_d"] is not None:
        init_d = np.array(c["init_d"])
        d_init_d = WD.dev(torch, init_d, np.int32)
    s = dict(positions=c["positions"], plans=None, current_goals=c["current_goals"], waypoints=c["waypoints"])
    _, d, _, _ = _compare(torch, grid, G, c["range"], s, F, init_d, d_field, d_init_d)
    assert d.tolist() == c["expect"]
    grid.close()
    wmap.close()


def test_wide_on_forest10_along_a_rollout(api, oracle, torch_cuda):
    import torch

    w = WC.forest10()
    wmap, grid = WD.device_grid(api, w)
    G = WC.reference_grid(oracle, w)
    F, init_d = R.mission_fields(G, w["starts"], w["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, w["starts"], w["goals"])
    n_updated, n_groups = 0, set()
    for s in WC.seeded_states(G, w, F, init_d, 30, 3.0, seed=3):
        g, _, u, _ = _compare(torch, grid, G, 3.0, s, F, init_d, d_field, d_init_d)
        n_updated += int(u.sum())
        n_groups.add(len(set(g.tolist())))
    assert n_updated > 30 and len(n_groups) > 1
    grid.close()
    wmap.close()


@pytest.mark.parametrize("n_agents", [64, 512])
def test_wide_on_random_forests(api, oracle, torch_cuda, n_agents):
    """One group (range -1, and 3 m), a few (2 m) and many (1 m: mostly agents alone); the group counts are the ones
    tests/test_waypoints_gpu.py asserts, so "one group" and "hundreds of groups" are both known to be exercised."""
    import torch

    w = WD.closed_loop().random_forest_world(64) if n_agents == 64 else WC.random_mission(512)
    wmap, grid = WD.device_grid(api, w)
    G = WC.reference_grid(oracle, w)
    F, init_d = R.mission_fields(G, w["starts"], w["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, w["starts"], w["goals"])
    seen = {}
    for rng in (-1, 3.0, 2.0, 1.0):
        for s in WC.seeded_states(G, w, F, init_d, 4 if n_agents == 64 else 2, rng, seed=11):
            g, _, _, _ = _compare(torch, grid, G, rng, s, F, init_d, d_field, d_init_d)
            seen[rng] = len(set(g.tolist()))
    assert seen[-1] == 1 and seen[1.0] > seen[3.0] >= 1 and seen[1.0] > n_agents // 8, seen
    assert n_agents == 64 or 1 < seen[2.0] < seen[1.0], seen
    grid.close()
    wmap.close()


# ---- hand-made swarms on an open 20 m x 20 m world around the origin (41 x 41 nodes, one pillar in a corner) -------------------------------
OPEN = {"boxes": [[9.0, 9.0, 1.25, 0.5, 0.5, 2.5]], "world_min": [-10.0, -10.0, 0.0], "world_max": [10.0, 10.0, 2.5], "resolution": 0.1,
        "max_dist": 1.0, "z_2d": 0.6, "radius": 0.15}
GOALS = [(-9.0, -9.0), (9.0, -9.0), (-9.0, 8.0), (0.0, 0.0), (5.0, -3.0), (-4.0, 6.0), (7.0, 2.0), (-7.0, -1.0)]  # (few: the restatement keeps one field per goal)


class _Open:
    """The open world on the device and in the restatement, made once for the module; fields per swarm."""

    def __init__(self, api, torch):
        self.torch = torch
        self.wmap, self.grid = WD.device_grid(api, OPEN)
        self.G = R.Grid(OPEN["world_min"], OPEN["world_max"], OPEN["z_2d"], 0.5, OPEN["radius"], occ=self.grid.download().astype(bool))
        assert self.G.dims[:2] == [41, 41] and 0 < self.G.occ.sum() < 20
        ys, xs = np.nonzero(~self.G.occ)
        self.free = np.c_[-10.0 + 0.5 * xs, -10.0 + 0.5 * ys, np.full(len(xs), OPEN["z_2d"])]

    def swarm(self, n, seed, waypoints=None):
        """n agents on distinct free nodes (or the given waypoints) with goals drawn from GOALS: the state dict without positions, the
        restatement's fields and the device's."""
        rnd = np.random.default_rng(seed)
        way = self.free[rnd.permutation(len(self.free))[:n]] if waypoints is None else np.array(waypoints, float)
        goals = np.array([list(GOALS[k]) + [OPEN["z_2d"]] for k in rnd.integers(0, len(GOALS), n)])
        F, init_d = R.mission_fields(self.G, list(way), list(goals))
        d_field, d_init_d = WD.device_fields(self.torch, self.grid, way, goals)
        assert np.array_equal(d_init_d.cpu().numpy(), init_d)
        way = f32(way).astype(float)
        return dict(plans=None, current_goals=way.copy(), waypoints=way), F, init_d, d_field, d_init_d


@pytest.fixture(scope="module")
def open_world(api, torch_cuda):
    import torch

    o = _Open(api, torch)
    yield o
    o.grid.close()
    o.wmap.close()


def _prev(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


@pytest.mark.parametrize("axis", ["x", "y", "diagonal"])
def test_cell_boundary(open_world, axis):
    """Range 4 m over the 20 m box: the cell side is 4.0004 m (5 x 5 = 25 cells <= 2 * 6 + 16, no enlargement), the cell edges lie at
    -10 + 4.0004 k = -5.9996, -1.9992, 2.0012, 6.0016.  Three pairs, each straddling an edge: exactly 4 m apart in float32 (`<` is strict:
    separate), one float32 ulp closer (one group), and exactly 4 m apart with one agent outside the world box (its cell index is clamped)."""
    o = open_world
    side = 1.0001 * 4.0
    assert (int(20.0 / side) + 1) ** 2 <= 2 * 6 + 16
    if axis == "diagonal":
        pos = [(-8.75, -8.75), (-4.75, -4.75), (0.25, 0.25), (_prev(4.25), _prev(4.25)), (10.75, -10.75), (6.75, -6.75)]
    else:
        pos = [(-8.75, -8.0), (-4.75, -8.0), (-8.75, 0.0), (_prev(-4.75), 0.0), (10.75, 8.0), (6.75, 8.0)]
        if axis == "y":
            pos = [(y, x) for x, y in pos]
    pos = np.array([[x, y, 0.6] for x, y in pos])
    assert np.array_equal(f32(pos[:, :2]).astype(float), pos[:, :2])
    for a, b in ((0, 1), (4, 5)):
        assert float(np.abs(f32(pos[a]) - f32(pos[b])).max()) == 4.0
    assert 0 < 4.0 - float(np.abs(f32(pos[2]) - f32(pos[3])).max()) < 1e-6
    for a, b in ((0, 1), (2, 3), (4, 5)):  # the pair lies in two different cells, along every axis it is apart on
        for k in range(2):
            ca, cb = (min(max(int(np.floor((pos[i][k] + 10.0) / side)), 0), 4) for i in (a, b))
            assert ca != cb or pos[a][k] == pos[b][k] or max(abs(pos[a][k]), abs(pos[b][k])) > 10.0, (a, b, k)
    s, F, init_d, d_field, d_init_d = o.swarm(6, seed=5)
    s["positions"] = pos
    g, _, _, _ = _compare(o.torch, o.grid, o.G, 4.0, s, F, init_d, d_field, d_init_d)
    assert g.tolist() == [0, 1, 2, 2, 4, 5]


def test_chain_of_200(open_world):
    """200 agents in a line 0.9 x range apart, ids shuffled: one group, named by its least id -- whatever order the pairs are hooked in.
    Without the middle agent: two groups.  (Range 0.1 m: 200 x 200 cells would be needed, so the side is enlarged until 416 cover the box
    and the line crosses about eighteen of them.)"""
    o = open_world
    rng = 0.1
    line = np.array([[float(f32(-9.0 + 0.9 * rng * k)), float(f32(0.3)), 0.6] for k in range(200)])
    perm = np.random.default_rng(7).permutation(200)
    s, F, init_d, d_field, d_init_d = o.swarm(200, seed=8)
    s["positions"] = line[perm]
    g, _, _, _ = _compare(o.torch, o.grid, o.G, rng, s, F, init_d, d_field, d_init_d)
    assert (g == 0).all()
    keep = perm != 100  # (the agent in the middle of the line leaves; the others keep their order, so ids shift down by one above it)
    s2, F2, init2, d_field2, d_init2 = o.swarm(199, seed=8, waypoints=s["waypoints"][keep])
    s2["positions"] = line[perm][keep]
    g2, _, _, _ = _compare(o.torch, o.grid, o.G, rng, s2, F2, init2, d_field2, d_init2)
    left = line[perm][keep][:, 0] < line[100, 0]
    assert len(set(g2.tolist())) == 2
    assert (g2[left] == np.nonzero(left)[0].min()).all() and (g2[~left] == np.nonzero(~left)[0].min()).all()


def test_two_groups_on_the_same_nodes(open_world):
    """Two groups far apart in position whose present waypoints lie on the SAME three nodes of a row, each group with a head-on conflict of
    its own: the node tables are per group, so neither sees the other's holders."""
    o = open_world
    row = [[-1.0, -2.0, 0.6], [-0.5, -2.0, 0.6], [0.0, -2.0, 0.6]]
    s, F, init_d, d_field, d_init_d = o.swarm(6, seed=3, waypoints=row + row)
    s["positions"] = np.array([[-8.0, -8.0, 0.6], [-7.5, -8.0, 0.6], [-8.0, -7.5, 0.6], [8.0, 8.0, 0.6], [7.5, 8.0, 0.6], [8.0, 7.5, 0.6]])
    g, d, _, _ = _compare(o.torch, o.grid, o.G, 2.0, s, F, init_d, d_field, d_init_d)
    assert g.tolist() == [0, 0, 0, 3, 3, 3]
    assert len(set(d[:3].tolist())) == 3 and len(set(d[3:].tolist())) == 3  # distinct within a group
    assert set(d[:3].tolist()) & set(d[3:].tolist())  # ... while the two groups take nodes of each other


def test_a_group_of_300_and_100_agents_alone(open_world):
    """One group of 300 (beyond a wavefront's 64 lanes, beyond the segment and the node table that stay in LDS below 256 members) next to
    100 agents alone, ids interleaved at random."""
    o = open_world
    rng = 0.5
    block = [[-9.5 + 0.4 * i, -9.5 + 0.4 * j, 0.6] for j in range(15) for i in range(20)]
    alone = [[-9.0 + 1.0 * i, 1.0 + 1.0 * j, 0.6] for j in range(9) for i in range(19)][:100]
    pos = f32(np.array(block + alone)).astype(float)
    perm = np.random.default_rng(12).permutation(400)
    s, F, init_d, d_field, d_init_d = o.swarm(400, seed=13)
    s["positions"] = pos[perm]
    g, _, _, _ = _compare(o.torch, o.grid, o.G, rng, s, F, init_d, d_field, d_init_d)
    sizes = sorted(np.bincount(g)[np.bincount(g) > 0].tolist())
    assert sizes == [1] * 100 + [300], sizes


def test_one_group_of_1000(open_world):
    o = open_world
    s, F, init_d, d_field, d_init_d = o.swarm(1000, seed=21)
    s["positions"] = s["waypoints"].copy()
    g, d, u, _ = _compare(o.torch, o.grid, o.G, -1.0, s, F, init_d, d_field, d_init_d)
    assert (g == 0).all() and len(set(d.tolist())) == 1000 and u.sum() > 0


def test_one_group_of_1100(open_world):
    """More members than a segment that is sorted in LDS holds (1024): the group's keys are sorted in their place in HBM."""
    o = open_world
    assert len(o.free) > 1660
    s, F, init_d, d_field, d_init_d = o.swarm(1100, seed=22)
    s["positions"] = s["waypoints"].copy()
    g, d, u, _ = _compare(o.torch, o.grid, o.G, -1.0, s, F, init_d, d_field, d_init_d)
    assert (g == 0).all() and len(set(d.tolist())) == 1100 and u.sum() > 0


def test_two_members_on_one_node(open_world):
    """PIBT's precondition broken: agents 0 and 2 of one group hold the same waypoint node.  The restatement is undefined there, so this
    case compares the two device entries only: the larger id is the node's holder in both."""
    o = open_world
    way = [[-1.0, -2.0, 0.6], [-0.5, -2.0, 0.6], [-1.0, -2.0, 0.6], [0.0, -2.0, 0.6]]
    s, F, init_d, d_field, d_init_d = o.swarm(4, seed=4, waypoints=way)
    s["positions"] = s["waypoints"].copy()
    for rng in (-1.0, 3.0):
        g, _, _, _ = _compare(o.torch, o.grid, o.G, rng, s, F, init_d, d_field, d_init_d, restatement=False)
        assert (g == 0).all()


def test_no_agent_one_agent_and_range_zero(api, open_world):
    import torch

    o = open_world
    s, F, init_d, d_field, d_init_d = o.swarm(1, seed=2)
    s["positions"] = s["waypoints"].copy()
    for rng in (-1.0, 0.0, 2.0):
        g, _, _, _ = _compare(torch, o.grid, o.G, rng, s, F, init_d, d_field, d_init_d)
        assert g.tolist() == [0]
    s, F, init_d, d_field, d_init_d = o.swarm(40, seed=6)
    s["positions"] = s["waypoints"].copy()
    g, _, _, _ = _compare(torch, o.grid, o.G, 0.0, s, F, init_d, d_field, d_init_d)
    assert g.tolist() == list(range(40))
    empty = torch.empty((0, 3), dtype=torch.float64, device="cuda")
    out = o.grid.waypoints_wide(3.0, 10, 2, torch.empty((0, 9), dtype=torch.float64, device="cuda"), None, empty, d_field, d_init_d, empty.clone())
    assert all(t.numel() == 0 for t in out)


def test_wide_argument_errors(api, open_world):
    import torch

    o = open_world
    s, F, init_d, d_field, d_init_d = o.swarm(4, seed=2)
    st = torch.zeros((4, 9), dtype=torch.float64, device="cuda")
    way = WD.dev(torch, s["waypoints"], np.float64)
    plan = torch.zeros((4, 120), dtype=torch.float64, device="cuda")
    with pytest.raises(api.LscqpError) as e:
        o.grid.waypoints_wide(3.0, 10, 3, st, None, way, d_field, d_init_d, way.clone())
    assert e.value.code == api.ERR_UNSUPPORTED and "2-D" in str(e.value)
    with pytest.raises(api.LscqpError) as e:
        o.grid.waypoints_wide(float("nan"), 10, 2, st, None, way, d_field, d_init_d, way.clone())
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "NaN" in str(e.value)
    with pytest.raises(api.LscqpError) as e:
        o.grid.waypoints_wide(3.0, 0, 2, st, plan, way, d_field, d_init_d, way.clone())
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    with pytest.raises(api.LscqpError) as e:
        o.grid.waypoints_wide(3.0, 10, 2, None, None, way, d_field, d_init_d, way.clone())
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    with pytest.raises(api.LscqpError) as e:
        o.grid.reserve_wide(-1)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert o.grid.status() == 0


@pytest.fixture(scope="module")
def forest512(api, oracle, torch_cuda):
    """WC.random_mission(512) on the device with one seeded state at range 2 m (some thirty groups and many agents alone)."""
    import torch

    w = WC.random_mission(512)
    wmap, grid = WD.device_grid(api, w)
    G = WC.reference_grid(oracle, w)
    F, init_d = R.mission_fields(G, w["starts"], w["goals"])
    d_field, d_init_d = WD.device_fields(torch, grid, w["starts"], w["goals"])
    s = WC.seeded_states(G, w, F, init_d, 2, 2.0, seed=11)[1]
    yield dict(grid=grid, s=s, d_field=d_field, d_init_d=d_init_d)
    grid.close()
    wmap.close()


def test_repeatable_and_scratch_clean(forest512):
    """Twenty calls on one input: all four outputs bit-identical (no result depends on the order in which atomics arrive).  Then 512
    agents, ten agents, and the 512 again on the same grid: the first and the last agree (nothing of a call survives into the next)."""
    import torch

    f = forest512
    grid, s = f["grid"], f["s"]
    first = _step(torch, grid, True, 2.0, s, f["d_field"], f["d_init_d"])
    assert 1 < len(set(first[0].tolist())) < 512 and first[2].sum() > 0
    for _ in range(19):
        again = _step(torch, grid, True, 2.0, s, f["d_field"], f["d_init_d"])
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    few = {k: (None if v is None else np.asarray(v)[:10]) for k, v in s.items()}
    ten_wide = _step(torch, grid, True, 2.0, few, f["d_field"][:10], f["d_init_d"][:10])
    ten_one = _step(torch, grid, False, 2.0, few, f["d_field"][:10], f["d_init_d"][:10])
    assert all(np.array_equal(a, b) for a, b in zip(ten_wide, ten_one))
    last = _step(torch, grid, True, 2.0, s, f["d_field"], f["d_init_d"])
    assert all(np.array_equal(a, b) for a, b in zip(first, last))


def test_captured_in_a_graph(forest512):
    """Reserved with reserve_wide, the call captures into a graph (nothing synchronises or allocates) and the replay gives the eager
    call's outputs."""
    import torch

    f = forest512
    grid, s = f["grid"], f["s"]
    n = len(s["waypoints"])
    eager = _step(torch, grid, True, 2.0, s, f["d_field"], f["d_init_d"])
    grid.reserve_wide(n)
    st = np.zeros((n, 9))
    st[:, :3] = s["positions"]
    d_st, d_plan, d_cg = WD.dev(torch, st), WD.dev(torch, WC.plan_from_points(np.asarray(s["plans"])), np.float64), WD.dev(torch, s["current_goals"], np.float64)
    d_way0 = WD.dev(torch, s["waypoints"], np.float64)
    d_way = d_way0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = grid.waypoints_wide(2.0, 10, 2, d_st, d_plan, d_cg, f["d_field"], f["d_init_d"], d_way)
    for _ in range(2):
        d_way.copy_(d_way0)
        for t in out:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in out] + [d_way.cpu().numpy().reshape(n, 3)]
        assert all(np.array_equal(a, b) for a, b in zip(eager, got))
    assert grid.status() == 0


def test_small_swarm_after_a_large_one(open_world):
    """A swarm of 300 fills the cells of a corner of the box; twelve agents in that same corner, on the same grid, right after it: the
    work arrays are laid out for the larger reservation and every cursor of the smaller call starts from zero all the same."""
    o = open_world
    big, Fb, ib, d_fb, d_ib = o.swarm(300, seed=31)
    big["positions"] = f32(np.array([[-9.5 + 0.4 * i, -9.5 + 0.4 * j, 0.6] for j in range(15) for i in range(20)])).astype(float)
    _compare(o.torch, o.grid, o.G, 0.5, big, Fb, ib, d_fb, d_ib)
    s, F, init_d, d_field, d_init_d = o.swarm(12, seed=32)
    s["positions"] = big["positions"][:12].copy()
    g, _, _, _ = _compare(o.torch, o.grid, o.G, 0.5, s, F, init_d, d_field, d_init_d)
    assert (g == 0).all()
