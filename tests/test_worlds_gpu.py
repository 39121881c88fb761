"""Each mission over its own world on the device (include/lscqp.h, "each mission over its own world"): the worlds form of the corridor
launch against the single-map entry run once per world, and a grid with a base occupancy per world against grids of each world and the
per-mission restatement (tests/world_cases.py).  Everything compared is the bits of a box, a status, an integer field or an exact grid
point: exact equality throughout, no tolerance."""
import numpy as np
import pytest

from tests import grid_reference as R
from tests import waypoint_device as WD
from tests import world_cases as WLD

pytestmark = pytest.mark.gpu
M, RADIUS = 5, 0.15
_REF = {}


def _maps(api, g, ks=range(WLD.N_WORLDS), **kw):
    args = dict(world_min=g["world_min"], world_max=g["world_max"], resolution=g["resolution"], max_dist=g["max_dist"])
    args.update(kw)
    return [api.WorldMap(g["worlds"][k], **args) for k in ks]


def _shared(api):
    """The fixture, a solver and the four fixture worlds as maps that are NEVER prepared (the single-map reference: every test evaluated),
    made once; a test that prepares maps makes its own."""
    if not _REF:
        g = WLD.fixture()
        _REF.update(g=g, sol=api.Solver(api.make_desc(M=M, dim=3, world_min=g["world_min"], world_max=g["world_max"])), maps=_maps(api, g))
    return _REF["g"], _REF["sol"], _REF["maps"]


def _pts(first, second=None, third=None):
    P = np.zeros((len(first), 3, 3))
    P[:, 0], P[:, 1], P[:, 2] = first, first if second is None else second, first if third is None else third
    return P


def _stages(api, pos, seed):
    """INIT, then three FROM_HULL and three FROM_POINT updates with moving points (float32 values, as the chain hands them over)."""
    n = len(pos)
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d[:, 2] = 0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    f32 = lambda a: np.float32(a).astype(np.float64)  # noqa: E731
    out = [(api.SFC_INIT, _pts(f32(pos)))]
    for s, mode in enumerate([api.SFC_FROM_HULL] * 3 + [api.SFC_FROM_POINT] * 3):
        step = 0.12 * (s + 1)
        out.append((mode, _pts(f32(pos + step * d), f32(pos + (step + 0.4) * d), f32(pos + (step + 0.3) * d))))
    return out


def _launch(api, torch, sol, n, mode, pts, boxes, where, world_of=None, order=None, cost=False):
    """One corridor launch: `where` a WorldMap (single-map entry) or a Worlds set with world_of.  (boxes, statuses, costs or None)"""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    d_sfc = up(boxes.view(np.float64).reshape(-1).copy())
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_cost = torch.zeros(n, dtype=torch.int32, device="cuda") if cost else None
    d_order = None if order is None else up(np.asarray(order, np.int32))
    d_r = up(np.full(n, RADIUS))
    if world_of is None:
        sol.construct_sfc_device(where, mode, n, up(pts.reshape(-1)), d_r, d_sfc, d_st, d_order=d_order, d_cost=d_cost)
    else:
        sol.construct_sfc_worlds_device(where, mode, n, up(np.asarray(world_of, np.int32)), up(pts.reshape(-1)), d_r, d_sfc, d_st, d_order=d_order, d_cost=d_cost)
    torch.cuda.synchronize()
    return d_sfc.cpu().numpy().view(api.BOX_DTYPE).reshape(n, M), d_st.cpu().numpy(), None if d_cost is None else d_cost.cpu().numpy()


def _reference_chains(api, torch, sol, maps, stages, pos):
    """Per world the whole chain of every agent through the single-map entry: per stage (input boxes, boxes, statuses).  An agent whose INIT
    failed goes on from the one-cell box round its position, so that every update has a box to start from."""
    n, res = len(pos), 0.1
    fallback = np.zeros((n, M), api.BOX_DTYPE)
    fallback["bmin"], fallback["bmax"] = (np.floor(pos / res) * res)[:, None, :], (np.ceil(pos / res) * res)[:, None, :]
    chains = []
    for mp in maps:
        state, rec = np.zeros((n, M), api.BOX_DTYPE), []
        for mode, pts in stages:
            boxes, st, _ = _launch(api, torch, sol, n, mode, pts, state, mp)
            rec.append((state, boxes, st))
            state = boxes.copy()
            if mode == api.SFC_INIT:
                state[st == 0] = fallback[st == 0]
        chains.append(rec)
    return chains


def _check_worlds_chain(api, torch, sol, ws, world_of, stages, chains, what):
    """Every stage of the worlds launch, fed the state the reference of the agent's own world left: boxes and statuses bit for bit; again with
    a reversed work order and the costs recorded."""
    n = len(world_of)
    pick = lambda s, j: np.stack([chains[world_of[a]][s][j][a] for a in range(n)])  # noqa: E731
    for s, (mode, pts) in enumerate(stages):
        inp, want, want_st = pick(s, 0), pick(s, 1), pick(s, 2)
        for order, cost in ((None, False), (np.arange(n)[::-1].copy(), True)):
            got, st, c = _launch(api, torch, sol, n, mode, pts, inp, ws, world_of=world_of, order=order, cost=cost)
            assert np.array_equal(st, want_st), (what, s, order is not None, np.nonzero(st != want_st))
            assert got.tobytes() == want.tobytes(), (what, s, order is not None)
            assert c is None or (c.view(np.uint32) > 0).all()


def _differs_from_world_0(chains, world_of):
    """Of the agents not in world 0: (how many, for how many INIT succeeds in their own world and in world 0, how many get a box in their own
    world that differs from what world 0 gives them -- where world 0 refuses the agent it gives no box, which differs).  From the single-map
    runs.  With the CPU oracle: 46 / 28 / 37 for the 64 agents, 194 / 112 / 144 for 257."""
    others = [a for a in range(len(world_of)) if world_of[a] != 0]
    both = [a for a in others if chains[0][0][2][a] == 1 and chains[world_of[a]][0][2][a] == 1]
    differ = [a for a in others if chains[world_of[a]][0][2][a] == 1 and chains[0][0][1][a].tobytes() != chains[world_of[a]][0][1][a].tobytes()]
    return len(others), len(both), len(differ)


def _world_of(n, seed=5):
    w = np.random.default_rng(seed).integers(0, WLD.N_WORLDS, n)
    if n > 8:
        assert (np.diff(w) < 0).any() and (np.diff(w) > 0).any() and len(set(w.tolist())) == WLD.N_WORLDS  # not monotonic, every world used
    return w.astype(np.int32)


@pytest.mark.parametrize("n", [1, 7, 64, "cus+1"])
def test_worlds_launch_equals_the_single_map_entry_per_world(api, torch_cuda, n):
    """Agent counts 1, 7, 64 and CUs + 1 (the last selects the throughput build), worlds prepared: INIT, three FROM_HULL and three FROM_POINT
    updates, a world index that is not monotonic, every agent against lscqp_construct_sfc_device on the map of its world."""
    torch = torch_cuda
    g, sol, ref_maps = _shared(api)
    n = torch.cuda.get_device_properties(0).multi_processor_count + 1 if n == "cus+1" else n
    pos = WLD.seeded_nodes(n, 2, g)
    stages = _stages(api, pos, 3)
    chains = _reference_chains(api, torch, sol, ref_maps, stages, pos)
    world_of = _world_of(n) if n > 1 else np.array([2], np.int32)
    maps = _maps(api, g)
    ws = api.Worlds(maps)
    assert ws.info()[0] == WLD.N_WORLDS and np.array_equal(ws.info()[1], maps[0].dims)
    ws.prepare(RADIUS)
    _check_worlds_chain(api, torch, sol, ws, world_of, stages, chains, "prepared")
    n_others, n_both, n_differ = _differs_from_world_0(chains, world_of)
    print("n = %d: %d agents outside world 0, INIT succeeds in both worlds for %d, the box differs for %d" % (n, n_others, n_both, n_differ))
    if n >= 64:  # the condition that keeps this test from passing with the index ignored
        assert 2 * n_differ >= n_others, (n_others, n_differ)
    ws.close()
    for m in maps:
        m.close()


@pytest.mark.parametrize("n", [64, "cus+1"])
@pytest.mark.parametrize("how", ["not_prepared", "one_member_at_another_margin", "one_member_prepared_behind_the_set"])
def test_worlds_launch_without_a_common_free_space_table(api, torch_cuda, how, n):
    """64 agents (the latency build) and CUs + 1 (the throughput build).  No member prepared; all prepared and then one again, directly, at a larger margin; and a set made from unprepared maps one of
    which is prepared afterwards (noticed through its generation counter): the launch uses no table and gives the same boxes."""
    torch = torch_cuda
    g, sol, ref_maps = _shared(api)
    n = torch.cuda.get_device_properties(0).multi_processor_count + 1 if n == "cus+1" else n
    pos = WLD.seeded_nodes(n, 2, g)
    stages = _stages(api, pos, 3)
    chains = _reference_chains(api, torch, sol, ref_maps, stages, pos)
    maps = _maps(api, g)
    ws = api.Worlds(maps)
    if how == "one_member_at_another_margin":
        ws.prepare(RADIUS)
        maps[2].prepare(0.4)
    world_of = _world_of(n)
    if how == "one_member_prepared_behind_the_set":
        _check_worlds_chain(api, torch, sol, ws, world_of, stages[:1], chains, how)
        maps[1].prepare(RADIUS)
    _check_worlds_chain(api, torch, sol, ws, world_of, stages, chains, how)
    ws.prepare(0.4)  # ... and with one margin for all again
    _check_worlds_chain(api, torch, sol, ws, world_of, stages[:3], chains, how + ", prepared again")
    ws.close()
    for m in maps:
        m.close()


def test_worlds_launch_statuses_and_boxes_equal_the_cpu_oracle(api, oracle, torch_cuda):
    """The 64-agent INIT launch against oracle.Map.construct_sfc per world, as tests/test_sfc.py does for one map."""
    torch = torch_cuda
    g, sol, ref_maps = _shared(api)
    n = 64
    pos = np.float32(WLD.seeded_nodes(n, 2, g)).astype(np.float64)
    world_of = _world_of(n)
    ws = api.Worlds(ref_maps)
    got, st, _ = _launch(api, torch, sol, n, api.SFC_INIT, _pts(pos), np.zeros((n, M), api.BOX_DTYPE), ws, world_of=world_of)
    ws.close()
    for k in range(WLD.N_WORLDS):
        omap = oracle.Map(g["worlds"][k], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
        want = np.zeros((n, M), oracle.BOX_DTYPE)
        st_w = omap.construct_sfc(oracle.SFC_INIT, _pts(pos), np.full(n, RADIUS), want)
        mine = world_of == k
        assert mine.any() and np.array_equal(st[mine], st_w[mine]), k
        ok = mine & (st_w == 1)
        assert ok.any() and np.array_equal(got["bmin"][ok], want["bmin"][ok]) and np.array_equal(got["bmax"][ok], want["bmax"][ok]), k


def test_degenerate_sets_equal_the_single_map_entry(api, torch_cuda):
    """A set of one world, and a set that lists one map twice."""
    torch = torch_cuda
    g, sol, ref_maps = _shared(api)
    n = 64
    pos = WLD.seeded_nodes(n, 2, g)
    stages = _stages(api, pos, 3)[:3]
    chains = _reference_chains(api, torch, sol, ref_maps[1:2], stages, pos)
    for members, world_of in (([ref_maps[1]], np.zeros(n, np.int32)), ([ref_maps[1], ref_maps[1]], (np.arange(n) % 2).astype(np.int32))):
        ws = api.Worlds(members)
        assert ws.info()[0] == len(members)
        _check_worlds_chain(api, torch, sol, ws, world_of, stages, [chains[0]] * len(members), "%d members" % len(members))
        ws.close()


def test_worlds_refusals(api, torch_cuda):
    torch = torch_cuda
    g, sol, ref_maps = _shared(api)
    for kw, field in ((dict(resolution=0.2), "resolution"), (dict(world_max=[5.0, 5.0, 3.0]), "world_max"), (dict(world_min=[-5.0, -6.0, 0.0]), "world_min"),
                      (dict(max_dist=0.5), "max_dist")):
        other = _maps(api, g, ks=[1], **kw)[0]
        with pytest.raises(api.LscqpError) as e:
            api.Worlds([ref_maps[0], ref_maps[2], other])
        assert e.value.code == api.ERR_INVALID_ARGUMENT and "map 2 differs from map 0 in " + field in str(e.value), (field, str(e.value))
        other.close()
    with pytest.raises(api.LscqpError) as e:
        api.Worlds([])
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "at least one world" in str(e.value)
    with pytest.raises(api.LscqpError) as e:
        api.Worlds([ref_maps[0], None])
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "map 1 is null" in str(e.value)
    ws = api.Worlds(ref_maps)
    n = 4
    d = torch.zeros(n * 9 * M, dtype=torch.float64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    with pytest.raises(api.LscqpError) as e:
        sol.construct_sfc_worlds_device(ws, api.SFC_INIT, n, None, d, d, d, d_st)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "null d_world_of" in str(e.value)
    with pytest.raises(api.LscqpError) as e:
        sol.construct_sfc_worlds_device(ws, 5, n, d_st, d, d, d, d_st)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "mode must be" in str(e.value)
    with pytest.raises(api.LscqpError) as e:
        ws.prepare(0.0)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    ws.close()


# ---- the grid --------------------------------------------------------------------------------------------------------------------------

def _compare_rollouts(api, torch, grid, Gs, w, off, starts, goals, ranges, steps, seed):
    """tests/test_missions_gpu.py::_compare_rollouts with a grid of its own per mission."""
    F, init_d = WLD.mission_fields(Gs, off, starts, goals)
    d_field, d_init_d = grid.fields_missions(off, WD.dev(torch, starts, np.float64), WD.dev(torch, goals, np.float64))
    torch.cuda.synchronize()
    assert np.array_equal(d_field.cpu().numpy(), F) and np.array_equal(d_init_d.cpu().numpy(), init_d)
    n_updated = 0
    for rng in ranges:
        states = WLD.seeded_states(Gs, off, w, starts, F, init_d, steps, rng, seed)
        for s in states:
            label, desired, updated, new = WLD.waypoint_step(Gs, off, rng, s["positions"], s["plans"], s["current_goals"], s["waypoints"], F, init_d)
            gr, d, u, way = WD.decision_step(torch, grid, rng, s, d_field, d_init_d, off=off)
            assert np.array_equal(d, desired), (rng, np.nonzero(d != desired))
            assert np.array_equal(gr, label) and np.array_equal(u, updated) and np.array_equal(way, new), rng
            n_updated += int(updated.sum())
    return n_updated, F


def test_grid_bases_fields_and_rollout_lds_tables(api, torch_cuda):
    """Three fixture worlds, missions of 10, 6 and 12 agents, node tables in LDS: every base equals the grid of that world alone; fields, init_d
    and ten rollout steps (range -1 and 3 m, five each) equal the restatement run per mission on that mission's own occupancy."""
    torch = torch_cuda
    g, _, ref_maps = _shared(api)
    w = WLD.world(0, g)
    off, starts, goals = WLD.seeded_missions([10, 6, 12], seed=1, g=g)
    grid = api.Grid(ref_maps[0], 0.5, g["radius"], g["z_2d"])
    assert 2 * int(grid.dims[0]) * int(grid.dims[1]) * 4 <= 60 * 1024
    ws = api.Worlds(ref_maps[:3])
    grid.set_worlds(ws)
    occs = []
    for k in range(3):
        alone = api.Grid(ref_maps[k], 0.5, g["radius"], g["z_2d"])
        occs.append(grid.download_world(k))
        assert np.array_equal(occs[k], alone.download()), k
        alone.close()
    assert not np.array_equal(occs[0], occs[1]) and not np.array_equal(occs[1], occs[2])
    assert np.array_equal(grid.download(), occs[0])  # (the one base of lscqp_grid_create is untouched)
    Gs = WLD.reference_grids(w, occs)
    n_updated, _ = _compare_rollouts(api, torch, grid, Gs, w, off, starts, goals, (-1, 3.0), 5, seed=23)
    assert n_updated > 10, n_updated
    # refusals: a partition of another size, the one-mission entries
    d_s, d_g = WD.dev(torch, starts, np.float64), WD.dev(torch, goals, np.float64)
    with pytest.raises(api.LscqpError) as e:
        grid.fields_missions([0, 10, 28], d_s, d_g)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and "3 worlds" in str(e.value) and "2 missions" in str(e.value)
    n = int(off[-1])
    zi = torch.zeros(n, dtype=torch.int32, device="cuda")
    zf = torch.zeros((n, int(grid.dims[1]), int(grid.dims[0])), dtype=torch.int32, device="cuda")
    for call in (lambda: grid.fields(d_s, d_g), lambda: grid.waypoints(3.0, 10, 2, WD.dev(torch, np.zeros((n, 9))), None, d_s, zf, zi, d_s.clone()),
                 lambda: grid.waypoints_wide(3.0, 10, 2, WD.dev(torch, np.zeros((n, 9))), None, d_s, zf, zi, d_s.clone())):
        with pytest.raises(api.LscqpError) as e:
            call()
        assert e.value.code == api.ERR_UNSUPPORTED and "lscqp_grid_set_worlds" in str(e.value)
    with pytest.raises(api.LscqpError):
        grid.download_world(3)
    # back to the one base
    grid.set_worlds(None)
    f1, _ = grid.fields(d_s[:30], d_g[:30])
    torch.cuda.synchronize()
    with pytest.raises(api.LscqpError):
        grid.download_world(0)
    grid.close()
    ws.close()


def test_grid_rollout_hbm_tables(api, torch_cuda):
    """Two synthetic forests on a 40 m side under a 0.25 m grid (161 x 161 nodes: the node tables of each mission in its slab of the HBM buffer),
    ten agents each: ten rollout steps against the restatement on each mission's own occupancy (taken from the device: its rule is tested above)."""
    torch = torch_cuda
    W = WLD.synthetic_worlds(2, side=40.0, n_boxes=300, seed=4)
    maps = [api.WorldMap(w["boxes"], w["world_min"], w["world_max"], w["resolution"], w["max_dist"]) for w in W]
    grid = api.Grid(maps[0], 0.25, W[0]["radius"], W[0]["z_2d"])
    assert 2 * int(grid.dims[0]) * int(grid.dims[1]) * 4 > 60 * 1024
    ws = api.Worlds(maps)
    grid.set_worlds(ws)
    occs = [grid.download_world(k) for k in range(2)]
    assert not np.array_equal(occs[0], occs[1])
    Gs = WLD.reference_grids(W[0], occs, resolution=0.25)
    starts, goals = [], []
    for k in range(2):  # ten start and ten goal nodes free in world k
        ys, xs = np.nonzero(~occs[k].astype(bool))
        pick = np.random.default_rng([9, k]).choice(len(xs), size=20, replace=False)
        p = np.array([Gs[k].point((int(xs[i]), int(ys[i]))) for i in pick], float)
        starts.append(p[:10])
        goals.append(p[10:])
    off = np.array([0, 10, 20])
    n_updated, _ = _compare_rollouts(api, torch, grid, Gs, W[0], off, np.concatenate(starts), np.concatenate(goals), (-1, 3.0), 5, seed=31)
    assert n_updated > 5, n_updated
    grid.close()
    ws.close()
    for m in maps:
        m.close()


def test_a_start_node_occupied_in_world_1_only_is_cleared_in_mission_1_only(api, torch_cuda):
    """Worlds (0, 1, 1) and three missions of one agent.  X is a node occupied in world 1 and free in world 0.  Mission 1 starts on X: it is
    opened in mission 1's copy only -- mission 2 flies over the same world 1 and still finds X occupied, mission 0 never had it occupied, and
    world 1's base keeps it."""
    torch = torch_cuda
    g, _, ref_maps = _shared(api)
    grid = api.Grid(ref_maps[0], 0.5, g["radius"], g["z_2d"])
    ws = api.Worlds([ref_maps[0], ref_maps[1], ref_maps[1]])
    grid.set_worlds(ws)
    occ0, occ1 = grid.download_world(0).astype(bool), grid.download_world(1).astype(bool)
    assert np.array_equal(grid.download_world(2).astype(bool), occ1)
    only1, both_free = np.argwhere(occ1 & ~occ0), np.argwhere(~occ1 & ~occ0)
    assert len(only1) and len(both_free) > 1
    G = R.Grid(g["world_min"], g["world_max"], g["z_2d"], 0.5, g["radius"], occ=occ0)
    pt = lambda ji: G.point((int(ji[1]), int(ji[0])))  # noqa: E731
    (j, i) = only1[0]
    X, free_a, free_b = pt(only1[0]), pt(both_free[0]), pt(both_free[-1])
    starts, goals = np.array([free_a, X, free_a], float), np.array([free_b, free_b, free_b], float)
    off = [0, 1, 2, 3]
    d_field, d_init = grid.fields_missions(off, WD.dev(torch, starts, np.float64), WD.dev(torch, goals, np.float64))
    torch.cuda.synchronize()
    Gs = WLD.reference_grids(WLD.world(0, g), [occ0, occ1, occ1])
    F, D = WLD.mission_fields(Gs, off, starts, goals)
    f = d_field.cpu().numpy()
    assert np.array_equal(f, F) and np.array_equal(d_init.cpu().numpy(), D)
    assert Gs[1].free[j, i] and not Gs[2].free[j, i] and Gs[0].free[j, i]
    assert f[2, j, i] == api.GRID_UNREACHABLE          # mission 2: X is an obstacle of its world
    assert f[1, j, i] == D[1] and f[1, j, i] != f[2, j, i]  # mission 1: X is its start node, open (init_d is the field there)
    assert f[0, j, i] == F[0, j, i] and not occ0[j, i]  # mission 0: never occupied in world 0 (whether its goal reaches X is the restatement's to say)
    assert grid.download_world(1)[j, i] == 1 and grid.download_world(0)[j, i] == 0  # the bases are what they were
    grid.close()
    ws.close()
