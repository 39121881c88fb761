"""The three kernels of a mission's own obstacles alone (include/lscqp.h, "a mission's own obstacles"; csrc/lscobstacle.hip:
obstacle_advance_kernel<true>, obstacle_drive_kernel<true>; csrc/lscpost.hip: safety_obstacles_kernel<true>), each against the entry of one
shared table (the <false> instantiation of the same text), run on one mission's slice (one agent's gathered sub-table) alone.  The single-table
entries are pinned on their own against tests/obstacle_reference.py, the oracle and lscqp_obstacle_drive_host.  A plan with one shared table
runs the <true> instantiations over one table and identity ids: the one-table cases here -- SHAPES' (65,) and the identity rows of the
safety leg -- hold them to what such a plan ran before.  Every comparison is exact equality of bytes; every byte that must not be written
holds a sentinel, guard entries behind the buffers included.  The shapes are tests/mission_obstacles_cases.py's."""
import numpy as np
import pytest

from tests import mission_obstacles_cases as MC

pytestmark = pytest.mark.gpu
GUARD = 0xA5


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _host(t, dtype):
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype)


def _guarded(torch, a, extra):
    """`a` on the device with `extra` guard bytes behind it."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([raw, np.full(extra, GUARD, np.uint8)])).cuda()


@pytest.fixture(scope="module")
def sol(api, torch_cuda):
    s = api.Solver(api.make_desc(M=5, dim=3))
    assert s.max_obstacles() >= 65
    yield s
    s.close()


def _clocks(K):
    return np.array(MC.CLOCKS[:K], np.int32)


@pytest.mark.parametrize("counts", MC.SHAPES, ids=["-".join(map(str, s)) for s in MC.SHAPES])
def test_the_advance_moves_each_slice_as_the_single_entry_does_by_its_own_clock(api, torch_cuda, sol, counts):
    """Each slice equals lscqp_obstacles_advance_device on that slice alone with that mission's clock -- 0, 7 and 400 -- and every clock comes
    back + 1, that of a mission without obstacles too.  HELD entries keep their sentinel bytes; so do the guards."""
    torch = torch_cuda
    K, off = len(counts), MC.offsets(counts)
    E = api.OBSTACLE_DTYPE.itemsize
    specs = [s for k, c in enumerate(counts) for s in MC.advance_specs(c, 20 + k)]
    models = api.obstacle_model_prepare(api.obstacle_models(specs)) if specs else np.zeros(0, api.OBSTACLE_MODEL_DTYPE)
    table0 = MC.table_at_reset(api, models)
    d_models, d_off = _guarded(torch, models, 8), _dev(torch, off)
    d_table, d_clock = _guarded(torch, table0, E), _guarded(torch, _clocks(K), 4)
    sol.obstacles_advance_missions_device(d_models, off, d_off, MC.TIME_STEP, d_clock, d_table)
    torch.cuda.synchronize()
    got, clocks = d_table.cpu().numpy(), _host(d_clock, np.int32)
    assert clocks[:K].tolist() == (_clocks(K) + 1).tolist() and clocks[K] == np.frombuffer(bytes([GUARD]) * 4, np.int32)[0]
    assert (got[len(models) * E:] == GUARD).all()
    moved = 0
    for k in range(K):
        lo, hi = int(off[k]), int(off[k + 1])
        if hi == lo:
            continue
        one_table, one_clock = _dev(torch, table0[lo:hi]), _dev(torch, _clocks(K)[k:k + 1])
        sol.obstacles_advance_device(_dev(torch, models[lo:hi]), hi - lo, MC.TIME_STEP, one_clock, one_table)
        torch.cuda.synchronize()
        want = one_table.cpu().numpy()
        assert got[lo * E:hi * E].tobytes() == want.tobytes(), (k, [i for i in range(hi - lo) if got[(lo + i) * E:(lo + i + 1) * E].tobytes() != want[i * E:(i + 1) * E].tobytes()][:8])
        assert _host(one_clock, np.int32)[0] == clocks[k]
        held = models["kind"][lo:hi] == api.OBSTACLE_HELD
        now = np.frombuffer(want.tobytes(), api.OBSTACLE_DTYPE)
        assert now[held].tobytes() == table0[lo:hi][held].tobytes()  # (sentinels and all)
        moved += int((now["type"][~held] == 0).sum())
    assert moved == int((models["kind"] != api.OBSTACLE_HELD).sum())


class Slices:
    """The per-mission references of the drive: every mission's slice as a table of its own, moved by the single-table entries on the
    device and, beside them, by lscqp_obstacle_drive_host."""

    def __init__(self, api, torch, sol, models, drives, hist, off, clocks, state, table0):
        self.api, self.torch, self.sol, self.hist, self.state, self.off = api, torch, sol, hist, state, off
        self.d_hist, self.d_state = (_dev(torch, hist) if len(hist) else None), (_dev(torch, state) if len(state) else None)
        self.parts = []
        for k in range(len(off) - 1):
            lo, hi = int(off[k]), int(off[k + 1])
            n = hi - lo
            self.parts.append(dict(n=n, models=models[lo:hi], drives=drives[lo:hi], d_models=_dev(torch, models[lo:hi]), d_drives=_dev(torch, drives[lo:hi]),
                                   d_table=_dev(torch, table0[lo:hi]), d_clock=_dev(torch, clocks[k:k + 1]),
                                   d_ckpt=torch.zeros(n * api.OBSTACLE_DRIVE_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                                   h_table=table0[lo:hi].copy(), h_ckpt=np.zeros(n, api.OBSTACLE_DRIVE_STATE_DTYPE), clock=int(clocks[k])))

    def drive(self):
        """One drive of every slice: (table bytes, checkpoint bytes) mission-major, the host's agreeing with the device's."""
        tabs, ckpts = [], []
        for q in self.parts:
            if q["n"]:
                self.sol.obstacles_drive_device(q["d_models"], q["d_drives"], q["n"], self.d_hist, len(self.hist), self.d_state, len(self.state), q["d_ckpt"],
                                                MC.TIME_STEP, q["d_clock"], q["d_table"])
                self.sol.obstacle_drive_host(q["models"], q["drives"], self.hist, self.state, q["h_ckpt"], MC.TIME_STEP, q["clock"], q["h_table"])
                self.torch.cuda.synchronize()
                assert q["d_table"].cpu().numpy().tobytes() == q["h_table"].tobytes() and q["d_ckpt"].cpu().numpy().tobytes() == q["h_ckpt"].tobytes()
            tabs.append(q["h_table"].tobytes())
            ckpts.append(q["h_ckpt"].tobytes())
        return b"".join(tabs), b"".join(ckpts)

    def advance(self):
        for q in self.parts:
            if q["n"]:
                self.sol.obstacles_advance_device(q["d_models"], q["n"], MC.TIME_STEP, q["d_clock"], q["d_table"])
                self.torch.cuda.synchronize()
                q["h_table"] = np.frombuffer(q["d_table"].cpu().numpy().tobytes(), self.api.OBSTACLE_DTYPE).copy()
            q["clock"] += 1
        return b"".join(q["h_table"].tobytes() for q in self.parts)


def _fly_drive(api, torch, sol, models, drives, hist, off, clocks, state, replans=2):
    """(drive, advance) `replans` times by the mission entries, held to the slices after every launch; returns the final table."""
    K, E, S = len(off) - 1, api.OBSTACLE_DTYPE.itemsize, api.OBSTACLE_DRIVE_STATE_DTYPE.itemsize
    n = len(models)
    table0 = MC.table_at_reset(api, models)
    ref = Slices(api, torch, sol, models, drives, hist, off, clocks, state, table0)
    d_models, d_drives, d_off = _guarded(torch, models, 8), _guarded(torch, drives, 8), _dev(torch, off)
    d_table, d_clock = _guarded(torch, table0, E), _guarded(torch, clocks, 4)
    d_ckpt = torch.cat([torch.zeros(n * S, dtype=torch.uint8, device="cuda"), torch.full((S,), GUARD, dtype=torch.uint8, device="cuda")])
    d_hist, d_state = (_dev(torch, hist) if len(hist) else None), (_dev(torch, state) if len(state) else None)
    for r in range(replans):
        sol.obstacles_drive_missions_device(d_models, d_drives, off, d_off, d_hist, len(hist), d_state, len(state), d_ckpt, MC.TIME_STEP, d_clock, d_table)
        torch.cuda.synchronize()
        want_table, want_ckpt = ref.drive()
        got, ck = d_table.cpu().numpy(), d_ckpt.cpu().numpy()
        assert got[:n * E].tobytes() == want_table, (r, [i for i in range(n) if got[i * E:(i + 1) * E].tobytes() != want_table[i * E:(i + 1) * E]][:8])
        assert ck[:n * S].tobytes() == want_ckpt, r
        assert (got[n * E:] == GUARD).all() and (ck[n * S:] == GUARD).all()
        assert _host(d_clock, np.int32)[:K].tolist() == (clocks + r).tolist()  # (the drive reads the clocks, the advance counts them)
        sol.obstacles_advance_missions_device(d_models, off, d_off, MC.TIME_STEP, d_clock, d_table)
        torch.cuda.synchronize()
        assert d_table.cpu().numpy()[:n * E].tobytes() == ref.advance(), r
    assert (_host(d_clock, np.int32)[K:] == np.frombuffer(bytes([GUARD]) * 4, np.int32)[0]).all()
    return np.frombuffer(d_table.cpu().numpy()[:n * E].tobytes(), api.OBSTACLE_DTYPE), table0


@pytest.mark.parametrize("counts", MC.SHAPES, ids=["-".join(map(str, s)) for s in MC.SHAPES])
def test_the_drive_moves_each_slice_as_the_single_entry_and_the_host_do(api, torch_cuda, sol, counts):
    """Two replans of (drive, advance) from clocks 0, 7 and 400 -- dt = 0 in one mission and > 0 in the others, a gaussian history not yet
    begun, under way, and long over; every gaussian obstacle of every mission reads the one shared slice of the history table; chasers after
    global agents and after goal points, each with neighbours of its own mission inside its avoiding distance."""
    n_total = 6
    off = MC.offsets(counts)
    models, drives, hist = MC.drive_tables(api, counts, n_total)
    if len(models) == 0:
        models = np.zeros(0, api.OBSTACLE_MODEL_DTYPE)
    last, first = _fly_drive(api, torch_cuda, sol, models, drives, hist, off, _clocks(len(counts)), MC.agent_states(n_total))
    driven = drives["kind"] != api.DRIVE_NONE
    if len(counts) > 1 and driven.any():
        later = np.zeros(len(models), bool)
        later[int(off[1]):] = True  # (missions 1, 2: clocks 7 and 400, dt > 0)
        if (driven & later).any():
            assert np.abs(last["position"][driven & later] - first["position"][driven & later]).max() > 1e-3
    plain = (models["kind"] == api.OBSTACLE_HELD) & ~driven
    assert last[plain].tobytes() == first[plain].tobytes()  # (an entry neither kernel moves keeps every sentinel byte)


def test_a_chaser_is_repelled_by_its_own_missions_obstacles_and_by_no_others(api, torch_cuda, sol):
    """Two missions, a chaser in each, the two chasers inside each other's avoiding distance and far from everything of their own mission:
    each flies as it does alone (the slices agree), and NOT as it does in one table of all four -- which is what a kernel that stages the
    whole table computes."""
    torch = torch_cuda
    models, drives, off = MC.neighbours_across_missions(api)
    clocks = np.array([3, 5], np.int32)
    hist, state = np.zeros((0, 3)), np.zeros((0, 9))
    last, first = _fly_drive(api, torch, sol, models, drives, hist, off, clocks, state, replans=3)
    assert np.abs(last["position"][[0, 2]] - first["position"][[0, 2]]).max() > 1e-3
    # one table of all four, both chasers by clock 3: chaser 0 is pushed off its course by chaser 2
    d_table, d_clock = _dev(torch, first), _dev(torch, clocks[:1])
    d_ckpt = torch.zeros(4 * api.OBSTACLE_DRIVE_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    alone_table, alone_clock = _dev(torch, first[:2]), _dev(torch, clocks[:1])
    sol.obstacles_drive_device(_dev(torch, models), _dev(torch, drives), 4, None, 0, None, 0, d_ckpt, MC.TIME_STEP, d_clock, d_table)
    sol.obstacles_drive_device(_dev(torch, models[:2]), _dev(torch, drives[:2]), 2, None, 0, None, 0, d_ckpt, MC.TIME_STEP, alone_clock, alone_table)
    torch.cuda.synchronize()
    shared, alone = _host(d_table, api.OBSTACLE_DTYPE), _host(alone_table, api.OBSTACLE_DTYPE)
    assert shared[0].tobytes() != alone[0].tobytes()


@pytest.fixture(scope="module")
def sub_tables(api, torch_cuda, sol):
    """Per agent count: the expected figures, made once by lscqp_safety_obstacles_device on each row's gathered sub-table."""
    torch, out = torch_cuda, {}
    for n in MC.SAFETY_AGENTS:
        c = MC.safety_case(api, n)
        d_x, d_r, d_w = _dev(torch, c["x"]), _dev(torch, c["radius"]), _dev(torch, c["downwash"])
        want = np.zeros(n, api.SAFETY_OBS_DTYPE)
        for p, row in enumerate(MC.ID_ROWS):
            slots = np.flatnonzero(row >= 0)
            d_one = torch.zeros(n * api.SAFETY_OBS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            sol.safety_obstacles_device(n, 0, n, 3, 0.07, d_x, d_r, d_w, len(slots), _dev(torch, c["table"][row[slots]]) if len(slots) else None, d_one)
            torch.cuda.synchronize()
            one = _host(d_one, api.SAFETY_OBS_DTYPE).copy()
            one["closest_obstacle"] = np.where(one["closest_obstacle"] >= 0, slots[np.maximum(one["closest_obstacle"], 0)] if len(slots) else -1, -1)
            mine = np.arange(n) % len(MC.ID_ROWS) == p
            want[mine] = one[mine]
        out[n] = (c, want)
    return out


@pytest.mark.parametrize("n", MC.SAFETY_AGENTS)
def test_the_safety_figures_by_ids_are_the_single_entrys_on_each_agents_gathered_sub_table(api, torch_cuda, sol, sub_tables, n):
    """-1 in front of, between and behind live ids; an exact tie between two slots (the lower slot wins, though it holds the higher table
    index); a REAL entry; a row that names nothing (+inf, -1, -1).  closest_obstacle is the slot.  The table lies one entry into its
    allocation and the record behind the last agent's is a guard."""
    torch = torch_cuda
    c, want = sub_tables[n]
    R, E = api.SAFETY_OBS_DTYPE.itemsize, api.OBSTACLE_DTYPE.itemsize
    d_out = torch.full(((n + 1) * R,), GUARD, dtype=torch.uint8, device="cuda")
    d_table = torch.cat([torch.full((E,), GUARD, dtype=torch.uint8, device="cuda"), _dev(torch, c["table"]), torch.full((E,), GUARD, dtype=torch.uint8, device="cuda")])
    sol.safety_obstacles_ids_device(n, 0, n, 3, 0.07, _dev(torch, c["x"]), _dev(torch, c["radius"]), _dev(torch, c["downwash"]), MC.N_SLOTS,
                                    _dev(torch, c["ids"]), len(c["table"]), d_table[E:], d_out)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    got = np.frombuffer(raw[:n * R].tobytes(), api.SAFETY_OBS_DTYPE)
    assert got.tobytes() == want.tobytes(), [a for a in range(n) if got[a].tobytes() != want[a].tobytes()][:8]
    assert (raw[n * R:] == GUARD).all()
    rows = np.arange(n) % len(MC.ID_ROWS)
    nothing = (MC.ID_ROWS[rows] < 0).all(1) | ((MC.ID_ROWS[rows] == MC.REAL) | (MC.ID_ROWS[rows] < 0)).all(1)
    assert np.isinf(got["safety_ratio_obs"][nothing]).all() and (got["closest_obstacle"][nothing] == -1).all() and (got["sample"][nothing] == -1).all()
    assert np.isfinite(got["safety_ratio_obs"][~nothing]).all()
    live = got["closest_obstacle"][~nothing]
    assert (c["ids"][~nothing][np.arange(len(live)), live] >= 0).all()  # a slot, and a live one
    if n >= 65:  # the tie is attained somewhere: the twins' lower slot, never the upper
        assert (got["closest_obstacle"][rows == 2] == 0).any() and not (got["closest_obstacle"][rows == 2] == 1).any()
        assert not (got["closest_obstacle"][rows == 3] == 4).any()
        assert (got["closest_obstacle"] != c["ids"][np.arange(n), np.maximum(got["closest_obstacle"], 0)])[~nothing].any()  # (not the table index)


def test_one_table_of_65_entries_is_among_the_shapes_of_the_advance_and_the_drive():
    """What a plan with one shared table launches: K = 1.  Both parametrisations above run MC.SHAPES."""
    assert (65,) in MC.SHAPES and len(MC.offsets((65,))) == 2


@pytest.mark.parametrize("n", (1, 65, 257))
def test_the_safety_figures_by_identity_ids_are_the_single_entrys_on_the_same_table(api, torch_cuda, sol, n):
    """Every agent's row 0 .. 6 over the seven entries of MC.safety_case (the REAL entry, the tied twins): what a plan with one shared table
    enqueues.  Byte for byte lscqp_safety_obstacles_device on that table -- the slot is the table index, the lower twin wins the tie."""
    torch = torch_cuda
    c = MC.safety_case(api, n)
    R, T = api.SAFETY_OBS_DTYPE.itemsize, len(c["table"])
    assert T == 7
    ids = np.ascontiguousarray(np.tile(np.arange(T, dtype=np.int32), (n, 1)))
    d_x, d_r, d_w, d_table = _dev(torch, c["x"]), _dev(torch, c["radius"]), _dev(torch, c["downwash"]), _dev(torch, c["table"])
    d_want = torch.zeros(n * R, dtype=torch.uint8, device="cuda")
    d_out = torch.full(((n + 1) * R,), GUARD, dtype=torch.uint8, device="cuda")
    sol.safety_obstacles_device(n, 0, n, 3, 0.07, d_x, d_r, d_w, T, d_table, d_want)
    sol.safety_obstacles_ids_device(n, 0, n, 3, 0.07, d_x, d_r, d_w, T, _dev(torch, ids), T, d_table, d_out)
    torch.cuda.synchronize()
    raw, want = d_out.cpu().numpy(), _host(d_want, api.SAFETY_OBS_DTYPE)
    assert raw[:n * R].tobytes() == want.tobytes(), [a for a in range(n) if raw[a * R:(a + 1) * R].tobytes() != want[a:a + 1].tobytes()][:8]
    assert (raw[n * R:] == GUARD).all()
    assert np.isfinite(want["safety_ratio_obs"]).all() and (want["closest_obstacle"] != MC.REAL).all() and (want["closest_obstacle"] != MC.TWIN_B).all()
