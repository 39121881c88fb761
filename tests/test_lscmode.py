"""The planner's other constraint generators (generateLSC / generateCLSC; plus generateBVC):
the oracle restatement (oracle/lscmode_oracle.c) against independent solutions and the reference's invariants, and the
HIP kernel against the oracle.  generateCLSC is what the reference's default launch runs (mode/planner = lsc with
mode/goal = grid_based_planner, reference src/traj_planner.cpp:551-553)."""
import numpy as np
import pytest

from tests import helpers as H

CLSC, BVC = 1, 2


def test_segment_segment_closest_points_against_exact_golden(oracle):
    """closestPointsBetweenLineSegments restated in the reference's float32 arithmetic vs the exact fp64 closest pair
    (tools/make_golden_segseg.py, 240 cases: generic, planar, parallel, degenerate, crossing)."""
    g = H.load_golden("segseg")
    worst_d = worst_p = 0.0
    for c in g["cases"]:
        d, c1, c2 = oracle.segseg_closest(c["l1s"], c["l1e"], c["l2s"], c["l2e"])
        worst_d = max(worst_d, abs(d - c["dist"]))
        if c["kind"] in ("generic", "planar", "degenerate1", "degenerate2"):  # unique closest pair
            worst_p = max(worst_p, np.abs(c1 - c["cp1"]).max(), np.abs(c2 - c["cp2"]).max())
        else:  # parallel / crossing: the pair is not unique (or ill conditioned); it must still be a closest pair
            assert abs(np.linalg.norm(c1 - c2) - c["dist"]) <= 2e-5
    # float32 procedure (points up to 3 m, a 3x3 float inverse) against an fp64 solution
    assert worst_d <= 2e-5 and worst_p <= 2e-4, (worst_d, worst_p)


def _swarm(N, M, dim, n_obs, seed):
    from lsc_dr_planner_amd import synth

    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=seed)
    b = sw.build()
    return sw, b


@pytest.mark.parametrize("N,M,dim,n_obs,seed", [(24, 5, 3, 8, 1), (12, 10, 2, 5, 2)])
def test_clsc_restatement_invariants(oracle, N, M, dim, n_obs, seed):
    sw, b = _swarm(N, M, dim, n_obs, seed)
    goal_all = np.ascontiguousarray(b["goal"], dtype=np.float64)
    init, nbr = b["init"], b["nbr"].astype(np.int32)
    L1 = oracle.generate_constraints(CLSC, init, nbr, sw.radius, sw.downwash, goal_all, dim=dim)
    L0 = oracle.generate_constraints(0, init, nbr, sw.radius, sw.downwash, goal_all, dim=dim)
    # segments m < M-1: generateCLSC = generateLSC whenever the hull does not contain the origin (:677-690 vs :618-657)
    for f in ("nrm", "d", "p"):
        assert np.array_equal(L1[f][:, :, :M - 1], L0[f][:, :, :M - 1]), f
    # last segment (:691-703): one point, one margin, one normal for the 6 control points; the agent's own last point and
    # its goal lie on the agent's side with slack (dist - (r_i + r_j)) / 2 by the closest-point property
    last = L1[:, :, M - 1]
    assert (last["d"] == last["d"][..., :1]).all() and (last["nrm"] == last["nrm"][..., :1, :]).all()
    dw = sw.downwash if dim == 3 else 1.0
    for a in range(N):
        for o in range(n_obs):
            r = last[a, o, 0]
            n_t = r["nrm"] * np.array([1, 1, dw])  # back in the transformed frame the normal is a unit vector
            if np.linalg.norm(r["nrm"]) < 1e-5:
                continue
            assert abs(np.linalg.norm(n_t) - 1) <= 1e-6
            dist = 2 * r["d"] - 2 * sw.radius
            for pt in (init[a, M - 1, 5] / np.array([1, 1, dw]), goal_all[a]):
                assert n_t @ (pt - r["p"]) >= dist - 2e-5, (a, o)
    # a pair sees mirrored last-segment constraints: n_ab = -n_ba, same margin
    for a in range(N):
        for o in range(n_obs):
            bb = nbr[a, o]
            where = np.nonzero(nbr[bb] == a)[0]
            if len(where):
                other = L1[bb, where[0], M - 1, 0]
                assert np.abs(other["nrm"] + last[a, o, 0]["nrm"]).max() <= 2e-6 and abs(other["d"] - last[a, o, 0]["d"]) <= 2e-6


def test_bvc_restatement_closed_form(oracle):
    sw, b = _swarm(16, 5, 3, 6, 3)
    goal_all = np.ascontiguousarray(b["goal"], dtype=np.float64)
    init, nbr = b["init"], b["nbr"].astype(np.int32)
    L = oracle.generate_constraints(BVC, init, nbr, sw.radius, sw.downwash, goal_all, dim=3)
    dw = sw.downwash
    for a in range(16):
        for o in range(6):
            diff = (init[a, 0, 0] - init[nbr[a, o], 0, 0]) / np.array([1, 1, dw])  # :716-718
            n = diff / np.linalg.norm(diff)
            want_d = 0.5 * (2 * sw.radius + np.linalg.norm(diff))  # :722-727
            want_n = n / np.array([1, 1, dw])  # :730
            assert np.abs(L[a, o]["nrm"] - want_n).max() <= 2e-7 and np.abs(L[a, o]["d"] - want_d).max() <= 2e-6
            assert np.array_equal(L[a, o]["p"], init[nbr[a, o]])  # :732-733: the neighbour's control points


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [CLSC, BVC, 0])
@pytest.mark.parametrize("N,M,dim,n_obs,seed", [(64, 5, 3, 20, 1), (10, 10, 2, 9, 2), (44, 10, 3, 40, 8)])
def test_gpu_generate_constraints_matches_oracle(api, oracle, mode, N, M, dim, n_obs, seed):
    import torch

    assert torch.cuda.is_available()
    sw, b = _swarm(N, M, dim, n_obs, seed)
    nbr = b["nbr"].astype(np.int32).copy()
    nbr[0, -1] = -1  # a missing neighbour -> zero rows
    init = b["init"].copy()
    init[1] = init[nbr[1, 0]]  # agent 1 sits exactly on its first neighbour: zero normals (CLSC) / fallback (LSC)
    goal_all = np.ascontiguousarray(b["goal"], dtype=np.float64).copy()
    goal_all[2] = init[2, M - 1, 5]  # agent 2 has arrived: degenerate (point) segment in the CLSC last-segment rows
    rad = np.full(N, sw.radius)
    dwv = np.full(N, sw.downwash)
    rad[3], dwv[3] = 0.2, 1.5  # heterogeneous pair: radius-weighted downwash (:1229-1240)
    L = oracle.generate_constraints(mode, init, nbr, rad, dwv, goal_all, dim=dim)
    want = api.pack_rows(L).reshape(N, n_obs, M, 6)
    dev = torch.device("cuda", 0)
    sol = api.Solver(api.make_desc(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_rows = torch.full((N * n_obs * M * 6 * 4,), float("nan"), dtype=torch.float64, device=dev)
    sol.generate_constraints_device(mode, N, n_obs, 0, up(init), up(nbr), up(rad), up(dwv), up(goal_all), d_rows)
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy().view(api.ROW_DTYPE).reshape(N, n_obs, M, 6)
    assert np.isfinite(d_rows.cpu().numpy()).all()
    assert (got["nx"][0, -1] == 0).all() and (got["b"][0, -1] == 0).all()
    # same float32 stages on both sides; the fp64 hull enumeration differs in operation order only (one float32 ulp on
    # the normal, 2e-6 on b = d + n.p); the float32 segment-segment procedure is restated without contraction on both
    # sides and agrees to the last bit except through sqrt/division rounding of the device (<= 1 ulp)
    for f, tol in (("nx", 2e-7), ("ny", 2e-7), ("nz", 2e-7), ("b", 2e-6)):
        assert np.abs(got[f] - want[f]).max() <= tol, (f, np.abs(got[f] - want[f]).max())


@pytest.mark.gpu
def test_gpu_sharded_constraints_use_global_goal_ids(api, oracle):
    """first_agent > 0: the local shard indexes trajectories, radii and goal points by global id."""
    import torch

    N, M, dim, n_obs = 40, 5, 3, 8
    sw, b = _swarm(N, M, dim, n_obs, 4)
    nbr = b["nbr"].astype(np.int32)
    goal_all = np.ascontiguousarray(b["goal"], dtype=np.float64)
    first, n_loc = 24, 16
    L = oracle.generate_constraints(CLSC, b["init"], nbr[first:], sw.radius, sw.downwash, goal_all, dim=dim, first_agent=first)
    want = api.pack_rows(L).reshape(n_loc, n_obs, M, 6)
    dev = torch.device("cuda", 0)
    sol = api.Solver(api.make_desc(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_rows = torch.zeros(n_loc * n_obs * M * 6 * 4, dtype=torch.float64, device=dev)
    sol.generate_constraints_device(CLSC, n_loc, n_obs, first, up(b["init"]), up(nbr[first:]), up(np.full(N, sw.radius)),
                                    up(np.full(N, sw.downwash)), up(goal_all), d_rows)
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy().view(api.ROW_DTYPE).reshape(n_loc, n_obs, M, 6)
    for f, tol in (("nx", 2e-7), ("ny", 2e-7), ("nz", 2e-7), ("b", 2e-6)):
        assert np.abs(got[f] - want[f]).max() <= tol, f


# ---- who is whose obstacle: broadcastMsgs' range filter (reference src/multi_sync_simulator.cpp:318-333) ---------------
def _numpy_neighbours(P, a, n_obs, rng_):
    d = np.abs(np.float32(P[a]) - np.float32(P)).max(1).astype(np.float64)
    ok = [j for j in range(len(P)) if j != a and not (rng_ > 0 and d[j] > rng_)]
    keep = sorted(sorted(ok, key=lambda j: (d[j], j))[:n_obs])
    return keep + [-1] * (n_obs - len(keep)), len(ok)


def test_neighbour_selection_oracle_against_numpy(oracle):
    rng = np.random.default_rng(3)
    P = np.float32(rng.uniform(-5, 5, (60, 3))).astype(np.float64)
    P[7] = P[3]  # coincident agents: distance 0
    for n_obs, rng_ in ((8, 3.0), (20, 3.0), (5, 0.0), (59, -1.0), (12, 1e-3)):
        nbr, cnt = oracle.select_neighbours(P, n_obs, rng_)
        for a in range(60):
            want, c = _numpy_neighbours(P, a, n_obs, rng_)
            assert list(nbr[a]) == want and cnt[a] == c, (n_obs, rng_, a)


@pytest.mark.gpu
@pytest.mark.parametrize("N,n_obs,comm_range,first,n_loc", [(300, 20, 3.0, 0, 300), (300, 6, 3.0, 100, 77), (130, 40, 0.0, 0, 130),
                                                            (64, 8, 1e-3, 0, 64), (4096, 20, 3.0, 1024, 512),
                                                            (1500, 8, 0.0, 700, 48)])  # > 1024 agents in range: the bisection path
def test_gpu_neighbour_selection_matches_oracle(api, oracle, N, n_obs, comm_range, first, n_loc):
    import torch

    rng = np.random.default_rng(N + n_obs)
    side = (N / 2.0) ** (1 / 3) * 2.5
    P = np.float32(rng.uniform(0, side, (N, 3))).astype(np.float64)
    P[first + 1] = P[first]  # coincident pair
    P[first + 2, 0] = P[first, 0] + 3.0  # exactly at the range in one axis (float32-exact): the reference's test is dist > range
    want, cnt = oracle.select_neighbours(P, n_obs, comm_range, first=first, n_agents=n_loc)
    dev = torch.device("cuda", 0)
    sol = api.Solver(api.make_desc(M=5, dim=3))
    d_nbr = torch.full((n_loc * n_obs,), -7, dtype=torch.int32, device=dev)
    d_cnt = torch.full((n_loc,), -7, dtype=torch.int32, device=dev)
    sol.select_neighbours_device(n_loc, first, N, n_obs, comm_range, torch.from_numpy(P).to(dev), d_nbr, d_cnt)
    torch.cuda.synchronize()
    assert np.array_equal(d_cnt.cpu().numpy(), cnt)
    assert np.array_equal(d_nbr.cpu().numpy().reshape(n_loc, n_obs), want)
    assert (cnt > n_obs).any() or comm_range == 1e-3 or n_obs >= 20  # the capacity rule is exercised in the small-n_obs cases


@pytest.mark.gpu
def test_bvc_mode_end_to_end_on_the_default_shape(api, oracle):
    """planner mode BVC on the reference's default shape (M = 10, 2-D): generateBVC rows from the device feed the QP without
    the LSC-mode end-stop rows (src/traj_optimizer.cpp:502-511 applies them in LSC mode only); the oracle re-solves from the
    same rows."""
    import torch

    N, M, dim, n_obs = 10, 10, 2, 9
    sw, b = _swarm(N, M, dim, n_obs, 2)
    dev = torch.device("cuda", 0)
    sol = api.Solver(api.make_desc(M=M, dim=dim, planner_mode=api.PLANNER_BVC, world_min=sw.world_min, world_max=sw.world_max))
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True, planner_lsc=False, world_min=sw.world_min, world_max=sw.world_max)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    goal_all = np.ascontiguousarray(b["goal"], dtype=np.float64)
    nbr = b["nbr"].astype(np.int32)
    d_rows = torch.zeros(N * n_obs * M * 6 * 4, dtype=torch.float64, device=dev)
    sol.generate_constraints_device(api.GEN_BVC, N, n_obs, 0, up(b["init"]), up(nbr), up(np.full(N, sw.radius)),
                                    up(np.full(N, sw.downwash)), up(goal_all), d_rows)
    hdr, _, off, sfc = api.batch_from_swarm(b, sw.n_obs, M)
    upb = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_x = torch.zeros(N * sol.nv, dtype=torch.float64, device=dev)
    d_obj = torch.zeros(N, dtype=torch.float64, device=dev)
    d_st = torch.full((N,), -1, dtype=torch.int32, device=dev)
    sol.solve_device(N, n_obs, upb(hdr), d_rows, upb(off), upb(sfc), d_x, d_obj, d_st)
    torch.cuda.synchronize()
    R = d_rows.cpu().numpy().view(api.ROW_DTYPE).reshape(N, n_obs, M, 6)
    x, obj, st = d_x.cpu().numpy().reshape(N, -1), d_obj.cpu().numpy(), d_st.cpu().numpy()
    assert (st == 0).all()
    for q in range(N):
        ag = oracle.make_agent(p0=hdr["p0"][q], v0=hdr["v0"][q], a0=hdr["a0"][q], goal=hdr["goal"][q], next_waypoint=hdr["next_waypoint"][q],
                               vmax=hdr["vmax"][q], amax=hdr["amax"][q], radius=hdr["radius"][q],
                               nominal_velocity=hdr["nominal_velocity"][q], n_obs=n_obs)
        lsc = np.zeros((n_obs, M, 6), oracle.LSC_DTYPE)
        lsc["nrm"][..., 0], lsc["nrm"][..., 1], lsc["nrm"][..., 2], lsc["d"] = R["nx"][q], R["ny"][q], R["nz"][q], R["b"][q]
        box = np.zeros(M, oracle.BOX_DTYPE)
        box["bmin"], box["bmax"] = b["sfc"]["bmin"][q], b["sfc"]["bmax"][q]
        o = oracle.solve(cls, ag, lsc, box)
        assert o["status"] == 0
        assert abs(o["obj"] - obj[q]) <= 1e-8 * max(1.0, abs(o["obj"])) and np.abs(o["x"] - x[q]).max() <= 1e-6, q
    # no end stop in BVC mode: some plan still moves at the end of the horizon
    X = x.reshape(N, dim, M, 6)
    assert np.abs(X[:, :, M - 1, 5] - X[:, :, M - 1, 4]).max() > 1e-4


# ---- generateCLSC on constructed hulls and on the segment-segment fixture (tests/lscgen_cases.py, tests/hull_reference.py) -------
@pytest.mark.gpu
@pytest.mark.parametrize("dim,M", [(3, 5), (2, 5), (3, 2)])
def test_gpu_generate_clsc_on_constructed_hulls(api, oracle, dim, M):
    """generate_lsc_kernel<CLSC>, segments m < M-1: the same closest-point search as generateLSC on every constructed family, held to
    the constructed result, the exact referee and the oracle.  No fallback here: a hull around the origin gives a zero normal and
    b = (r_a + r_b) / 2 exactly, and a hull closer than 1e-5 m keeps its own normal (both stated by construction)."""
    from tests import lscgen_cases as LC
    from tests import lscgen_checks as T

    cases, _, n_ref, n_con = LC.suite(dim)
    pk = LC.pack_pairs(cases, M, dim, hull_segments=M - 1)
    got = LC.run_pairs_device(api, CLSC, pk)
    T._hold_device(cases, pk, got, LC.oracle_pairs(oracle, api, CLSC, pk), n_con, n_ref, "clsc", lambda n: LC.expected_for_pack(cases, pk, n, "clsc"))
    T._coverage_line(cases, pk, dim, "generate_clsc (M=%d)" % M)


@pytest.mark.gpu
def test_gpu_clsc_last_segment_on_the_segment_segment_fixture(api, oracle):
    """The 240 cases of tests/golden/segseg.json (generic, planar, parallel, degenerate, crossing) through segseg_closest ON THE DEVICE:
    the neighbour's last point and goal are segment 1, the agent's are segment 2 (M = 2, downwash 1).  Rows against the oracle at the
    standing bars; the distance recovered from the rows, 2 d - (r_a + r_b) with d = b - n . p, against the fixture's exact distance
    at the fixture's 2e-5 bar."""
    from tests import lscgen_cases as LC

    g = H.load_golden("segseg")["cases"]
    N, M, r = len(g), 2, 0.15
    assert N == 240
    traj = np.zeros((2 * N, M, 6, 3))
    goal_all = np.zeros((2 * N, 3))
    for a, c in enumerate(g):
        traj[a, :, :] = np.float32(c["l2s"])
        traj[N + a, :, :] = np.float32(c["l1s"])
        traj[a, 0] += 16.0  # segment 0: two separated points (a hull case of no interest here)
        goal_all[a], goal_all[N + a] = np.float32(c["l2e"]), np.float32(c["l1e"])
    pk = dict(N=N, M=M, dim=3, traj=traj, nbr=(N + np.arange(N, dtype=np.int32)).reshape(N, 1), radius=np.full(2 * N, r), downwash=np.ones(2 * N),
              goal_all=goal_all)
    got = LC.run_pairs_device(api, CLSC, pk)
    L = oracle.generate_constraints(CLSC, traj, pk["nbr"], pk["radius"], pk["downwash"], goal_all, dim=3)
    want = LC.oracle_pairs(oracle, api, CLSC, pk)
    dn, db = np.abs(got - want)[..., :3].max(), np.abs(got - want)[..., 3].max()
    print("segseg through CLSC: device vs oracle normal %.3g b %.3g" % (dn, db))
    assert dn <= 2e-7 and db <= 2e-6, (dn, db)
    last = got[:, M - 1]  # (N, 6, 4): one normal, one point, one margin for the six control points
    assert (last == last[:, :1]).all()
    p = L["p"][:, 0, M - 1, 0]  # the oracle's closest point on segment 1 (the device does not return it)
    d = last[:, 0, 3] - (last[:, 0, :3] * p).sum(-1)
    dist = 2 * d - 2 * r
    worst = np.abs(dist - np.array([c["dist"] for c in g])).max()
    print("segseg through CLSC: recovered distance vs exact %.3g" % worst)
    assert worst <= 2e-5, worst
    # the oracle itself says the same of these pairs (segseg_closest, as test_segment_segment_closest_points_against_exact_golden holds it)
    for a in (0, 100, 239):
        dd, c1, _ = oracle.segseg_closest(g[a]["l1s"], g[a]["l1e"], g[a]["l2s"], g[a]["l2e"])
        assert abs((2 * L["d"][a, 0, M - 1, 0] - 2 * r) - dd) <= 1e-12 and np.array_equal(c1, p[a])
