"""generate_clsc_obstacle_kernel alone (csrc/lscgen.hip, lscqp_generate_obstacle_rows_device in LSCQP_GEN_CLSC mode) on the device: the
constructed packs of tests/obstacle_clsc_cases.py in both row formats, equality with the agent kernel on the equivalent agent pair, the
last segment on the segment-segment fixture, the launch shapes around the workgroup size, the remapped store, and LSCQP_GEN_LSC through
the new entry."""
import numpy as np
import pytest

from tests import helpers as H
from tests import lscgen_cases as LC
from tests import lscgen_checks as T
from tests import obstacle_clsc_cases as OC
from tests.test_obstacle_clsc_cpu import STATIC, hold_rows, zero_rows_hold

pytestmark = pytest.mark.gpu

CLSC = 1


@pytest.fixture(scope="module")
def static_packs(oracle):
    out = {}
    for suite, dim, tall in STATIC:
        cases, _, n_ref, n_con = LC.suite(suite)
        pk = OC.pack_static(cases, 6, dim, tall=tall)
        out[(suite, dim, tall)] = (cases, n_ref, n_con, pk, OC.restatement(oracle, pk))
    return out


def agent_kernel_rows(api, pk, rows_f32=False):
    return LC.run_pairs_device(api, CLSC, OC.as_agent_pairs(pk), rows_f32=rows_f32)


@pytest.mark.parametrize("rows_f32", [False, True], ids=["f64", "rows_f32"])
@pytest.mark.parametrize("key", STATIC, ids=["3d", "2d", "tall"])
def test_constructed_packs(api, torch_cuda, static_packs, key, rows_f32):
    """Held to the constructed result, the referee's normals and the restatement at TOL_N / TOL_B (TOL_B_F32 under LSCQP_ROWS_F32); slivers
    to the referee at their own bar; zero rows and n_z == 0 with ==; every hull feature wins somewhere."""
    cases, n_ref, n_con, pk, rest = static_packs[key]
    got = OC.run_device(api, pk, rows_f32=rows_f32)
    hold_rows(cases, pk, got, rest, n_con, n_ref, rows_f32=rows_f32)
    assert zero_rows_hold(cases, pk, got) > 0
    T._coverage_line(cases, pk, key[0], "generate_clsc_obstacle (%s%s)" % ("tall, " if key[2] else "", "rows_f32" if rows_f32 else "f64"))


@pytest.mark.parametrize("key", STATIC[:2], ids=["3d", "2d"])
def test_non_tall_packs_equal_the_agent_kernel_exactly(api, torch_cuda, oracle, static_packs, key):
    """3-D: every segment.  2-D: the hull segments -- on the last one these packs separate (obstacle -> the origin, off the plane z = 0.6)
    from (agent -> goal), the record's normal has a z component, and the obstacle kernel writes the 2-D QP's row (n_z = 0, b = d + n_x p_x
    + n_y p_y) where the agent kernel, whose pairs have both goals in the plane, packs all three terms: held there to the agent oracle's
    unpacked records at TOL_N / TOL_B."""
    pk = static_packs[key][3]
    hull = slice(None) if pk["dim"] == 3 else slice(0, pk["M"] - 1)
    for rows_f32 in (False, True):
        got = OC.run_device(api, pk, rows_f32=rows_f32)
        assert np.array_equal(got[:, hull], agent_kernel_rows(api, pk, rows_f32)[:, hull]), rows_f32
        if pk["dim"] == 2:
            want, rec_n = OC.agent_oracle_rows(oracle, pk)
            T._hold(got, want, T.TOL_N, T.TOL_B_F32 if rows_f32 else T.TOL_B, what="device 2-D static pack vs agent oracle's records")
            assert (got[..., 2] == 0).all() and (np.abs(rec_n[:, pk["M"] - 1, 2]) > 1e-3).sum() >= pk["N"] // 4


@pytest.mark.parametrize("dim,M", [(3, 5), (3, 2), (2, 5), (2, 2)])
def test_moving_obstacles_equal_the_agent_kernel_exactly_and_the_restatement(api, torch_cuda, oracle, dim, M):
    """Velocity != 0 and explicit obstacle goal points.  Non-tall obstacles: == the device's own generate_constraints_device(GEN_CLSC) on
    the equivalent agent pair (the same device functions on the same float32 values); all of them, tall ones included: the restatement
    at TOL_N / TOL_B."""
    pk = OC.pack_moving(M, dim, n=24)
    got = OC.run_device(api, pk)
    T._hold(got, OC.restatement(oracle, pk), what="device moving %d-D M=%d vs restatement" % (dim, M))
    twin = agent_kernel_rows(api, pk)
    keep = ~pk["tall_mask"]
    assert keep.sum() >= 12 and np.array_equal(got[keep], twin[keep])
    if dim == 3 and M > 1:
        assert (got[pk["tall_mask"], :M - 1, :, 2] == 0).all() and (np.abs(got[pk["tall_mask"], :M - 1, :, :2]).max(-1) > 0).all()
    else:  # 2-D: the tall rule changes nothing (every z is z_2d already)
        assert np.array_equal(got, twin)


def test_last_segment_on_the_segment_segment_fixture(api, torch_cuda, oracle):
    """The 240 cases of tests/golden/segseg.json: rows against the agent oracle at the bars tests/test_lscmode.py holds the agent branch to
    (2e-7, 2e-6), the distance recovered from the rows against the fixture's exact one at its 2e-5 bar, and == the agent kernel."""
    g = H.load_golden("segseg")["cases"]
    assert len(g) == 240
    pk = OC.pack_segseg(g)
    N, M, r = pk["N"], pk["M"], 0.15
    got = OC.run_device(api, pk)
    pairs = OC.as_agent_pairs(pk)
    want = LC.oracle_pairs(oracle, api, CLSC, pairs)
    dn, db = np.abs(got - want)[..., :3].max(), np.abs(got - want)[..., 3].max()
    print("segseg through the obstacle kernel: device vs oracle normal %.3g b %.3g" % (dn, db))
    assert dn <= 2e-7 and db <= 2e-6, (dn, db)
    last = got[:, M - 1]
    assert (last == last[:, :1]).all()
    L = oracle.generate_constraints(CLSC, pairs["traj"], pairs["nbr"], pairs["radius"], pairs["downwash"], pairs["goal_all"], dim=3)
    p = L["p"][:, 0, M - 1, 0]
    dist = 2 * (last[:, 0, 3] - (last[:, 0, :3] * p).sum(-1)) - 2 * r
    worst = np.abs(dist - np.array([c["dist"] for c in g])).max()
    print("segseg through the obstacle kernel: recovered distance vs exact %.3g" % worst)
    assert worst <= 2e-5, worst
    for a in (0, 100, 239):
        dd, c1, _ = oracle.segseg_closest(g[a]["l1s"], g[a]["l1e"], g[a]["l2s"], g[a]["l2e"])
        assert abs((2 * L["d"][a, 0, M - 1, 0] - 2 * r) - dd) <= 1e-12 and np.array_equal(c1, p[a])
    assert np.array_equal(got, agent_kernel_rows(api, pk))
    # M = 1: every unit is a last segment
    pk1 = OC.pack_segseg(g, M=1)
    got1 = OC.run_device(api, pk1)
    assert got1.shape == (N, 1, 6, 4) and np.array_equal(got1[:, 0], last)


def test_null_obstacle_goals_are_an_all_zero_table(api, torch_cuda, oracle):
    """d_obstacle_goal = NULL is the origin for every obstacle (what the plan passes); M = 2 and M = 5, 3-D and 2-D"""
    for dim, M in ((3, 2), (3, 5), (2, 5)):
        pk = OC.pack_moving(M, dim, n=12, seed=5)
        a, b = OC.run_device(api, pk, goals=None, raw=True), OC.run_device(api, pk, goals="zeros", raw=True)
        assert a.tobytes() == b.tobytes()
        rows = LC.rows_array(a, api, False, (pk["N"], 1, M, 6))[:, 0]
        origin = dict(pk, obstacle_goal=None)
        T._hold(rows, OC.restatement(oracle, origin), what="device NULL goals %d-D M=%d vs restatement" % (dim, M))
        if dim == 2:
            # the plane is z = 0.6, the origin off it: the row is d + n_x p_x + n_y p_y of the unpacked record, n_z = 0, and the three-term
            # packing would be centimetres off
            want, rec_n = OC.agent_oracle_rows(oracle, origin)
            T._hold(rows, want, what="device NULL goals 2-D vs agent oracle's records")
            assert (rows[..., 2] == 0).all() and (np.abs(rec_n[:, M - 1, 2]) > 1e-2).sum() >= 3
            three = LC.oracle_pairs(oracle, api, CLSC, OC.as_agent_pairs(origin))
            assert np.abs(three[:, M - 1, :, 3] - rows[:, M - 1, :, 3]).max() > 1e-2
        assert a.tobytes() != OC.run_device(api, pk, raw=True).tobytes()  # (the pack's own goal points are read when given)


@pytest.mark.parametrize("n_units", [1, 255, 256, 257, 513])
def test_launch_shapes_around_the_workgroup(api, torch_cuda, n_units):
    """kThreads = 256: one lane, one short of a block, a block, one over, two blocks and a lane (M = 1, so n_units = n_agents); every unit
    equals the same unit of the largest launch."""
    big = OC.pack_moving(1, 3, n=513, seed=9)
    ref = _shape_reference(api, big)
    pk = {k: (v[:n_units] if isinstance(v, np.ndarray) and v.shape[:1] == (513,) else v) for k, v in big.items()}
    pk["N"] = n_units
    got = OC.run_device(api, pk)
    assert np.array_equal(got, ref[:n_units]) and np.abs(got[..., :3]).max(-1).min() > 0


_SHAPE_REF = {}


def _shape_reference(api, big):
    if "rows" not in _SHAPE_REF:
        _SHAPE_REF["rows"] = OC.run_device(api, big)
    return _SHAPE_REF["rows"]


def test_first_agent_and_empty_slots(api, torch_cuda):
    """first_agent > 0: trajectories and radii are read by global id, goals and ids by local id.  id < 0: six all-zero rows."""
    pk = OC.pack_moving(3, 3, n=40, seed=11)
    whole = OC.run_device(api, pk)
    part = OC.run_device(api, pk, first_agent=17, n_agents=20)
    assert np.array_equal(part, whole[17:37])
    ids = pk["ids"].copy()
    ids[::3] = -1
    holes = OC.run_device(api, pk, ids=ids)
    assert (holes[::3] == 0).all() and np.array_equal(np.delete(holes, np.s_[::3], 0), np.delete(whole, np.s_[::3], 0))
    # two slots per agent, the second one empty or another agent's obstacle
    two = np.stack([pk["ids"][:, 0], np.where(np.arange(40) % 2 == 0, -1, (pk["ids"][:, 0] + 1) % 40)], axis=1).astype(np.int32)
    buf = OC.run_device(api, pk, ids=two, n_obs_total=2, raw=True)
    rows = LC.rows_array(buf, api, False, (40, 2, 3, 6))
    assert np.array_equal(rows[:, 0], whole) and (rows[::2, 1] == 0).all() and (np.abs(rows[1::2, 1, :, :, :3]).max(-1) > 0).all()


@pytest.mark.parametrize("rows_f32", [False, True], ids=["f64", "rows_f32"])
def test_remapped_store_touches_its_own_slot_only(api, torch_cuda, rows_f32):
    """Slot 1 of 3: every byte of slots 0 and 2 still holds the 0xFF sentinel, slot 1 holds the rows of the plain launch."""
    pk = OC.pack_moving(3, 3, n=90, seed=13)  # 270 units: two workgroups
    item = 16 if rows_f32 else 32
    plain = OC.run_device(api, pk, rows_f32=rows_f32, raw=True).reshape(pk["N"], 1, -1)
    buf = OC.run_device(api, pk, rows_f32=rows_f32, n_obs_total=3, slot0=1, raw=True).reshape(pk["N"], 3, pk["M"] * 6 * item)
    assert (buf[:, 0] == 0xFF).all() and (buf[:, 2] == 0xFF).all()
    assert buf[:, 1].tobytes() == plain[:, 0].tobytes() and not (plain == 0xFF).all(-1).any()


def test_mode_lsc_is_the_lsc_entry_bit_for_bit(api, torch_cuda):
    """LSCQP_GEN_LSC through the new entry launches lscqp_generate_lsc_obstacles_device's kernel with its arguments: the same bytes on
    tests/lscgen_cases.pack_obstacles, in both row formats."""
    cases = LC.suite(3)[0]
    pk = LC.pack_obstacles(cases, 5, 3)
    for rows_f32 in (False, True):
        want = LC.run_obstacles_device(api, pk, rows_f32=rows_f32)
        got = OC.run_device(api, dict(pk, obstacle_goal=None), mode=api.GEN_LSC, rows_f32=rows_f32)
        assert np.array_equal(got, want) and np.abs(want).max() > 0
