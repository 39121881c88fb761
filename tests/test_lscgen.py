"""LSC generation: the oracle restatement against the REFERENCE's openGJK, and the HIP kernel
against the oracle.  Tolerances are stated where they are used."""
import os

import numpy as np
import pytest

from tests import helpers as H


def test_hull_closest_point_against_reference_gjk_golden(oracle):
    """Committed outputs of the reference's own openGJK (tools/make_golden_gjk.py): distance and closest point of 240
    six-point hulls (generic, planar, repeated points, float32 coordinates, origin inside)."""
    g = H.load_golden("gjk_hulls")
    worst = 0.0
    for c in g["cases"]:
        d, p = oracle.hull_closest_point(np.array(c["hull"]))
        worst = max(worst, abs(d - c["dist"]), np.abs(p - np.array(c["closest"])).max())
    assert worst <= 1e-9, worst  # both are fp64 solutions of the same unique projection


def test_hull_closest_point_against_reference_gjk_live(oracle):
    """Same check on 3000 further hulls (generic, planar, two repeated points) against the outputs of the reference's openGJK recorded
    for them (tools/make_golden_gjk.py -> gjk_hulls_3000.npz)."""
    g = np.load(os.path.join(H.GOLDEN, "gjk_hulls_3000.npz"))
    assert g["hull"].shape == (3000, 6, 3)
    worst = 0.0
    for pts, dr, v in zip(g["hull"], g["dist"], g["closest"]):
        d, p = oracle.hull_closest_point(pts)
        worst = max(worst, abs(d - dr), np.abs(p - v).max())
    assert worst <= 1e-9, worst


def _swarm_inputs(N, M, dim, n_obs, seed):
    from lsc_dr_planner_amd import synth

    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=seed)
    b = sw.build()
    return sw, b


@pytest.mark.parametrize("N,M,dim,n_obs,seed", [(24, 5, 3, 8, 1), (12, 10, 2, 5, 2)])
def test_generate_lsc_restatement_matches_independent_numpy_and_invariants(oracle, N, M, dim, n_obs, seed):
    sw, b = _swarm_inputs(N, M, dim, n_obs, seed)
    L = oracle.generate_lsc(b["init"], b["nbr"], sw.radius, sw.downwash, b["goal"], dim=dim)
    # (a) the workload generator's numpy restatement (written independently, vectorised): float32 staging -> 2e-7
    for f in ("p", "nrm", "d"):
        assert np.abs(L[f] - b["lsc"][f]).max() <= 2e-7, f
    # (b) the feasibility invariant of SURVEY.md section 8d: the agent's own initial control point satisfies its row with
    #     slack 1/2 (rel.n - (r_i + r_j)) >= 0 when the hulls are collision free
    own = b["init"][:, None]  # (N,1,M,6,3)
    slack = np.einsum("nkmic,nkmic->nkmi", own - L["p"], L["nrm"]) - L["d"]
    assert slack.min() >= -1e-6
    # (c) the neighbour's row is the mirror image: -normal (3-D normals are unit in downwash-scaled coordinates)
    for a in range(N):
        for oi, j in enumerate(b["nbr"][a]):
            back = np.where(b["nbr"][j] == a)[0]
            if len(back):
                assert np.abs(L["nrm"][a, oi] + L["nrm"][j, back[0]]).max() <= 2e-7


def test_generate_lsc_fallback_when_hulls_overlap(oracle):
    """Hull of the relative control points contains the origin -> normal = (goal - obstacle position) normalised,
    reference src/traj_planner.cpp:624-633."""
    M = 3
    traj = np.zeros((2, M, 6, 3))
    rng = np.random.default_rng(3)
    traj[0] = np.float32(rng.normal(size=(M, 6, 3)) * 0.5)
    traj[1] = np.float32(rng.normal(size=(M, 6, 3)) * 0.5)
    goal = np.array([[3.0, 4.0, 0.0]])
    L = oracle.generate_lsc(traj, np.array([[1]]), 0.15, 1.0, goal, dim=3)
    for m in range(M):
        rel = np.float32(traj[0, m]) - np.float32(traj[1, m])
        d, _ = oracle.hull_closest_point(rel.astype(np.float64))
        if d == 0.0:
            fb = goal[0] - traj[1, 0, 0]
            assert np.abs(L["nrm"][0, 0, m, 0] - fb / np.linalg.norm(fb)).max() <= 2e-7


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,M,dim,n_obs,seed", [(64, 5, 3, 20, 1), (10, 10, 2, 9, 2), (48, 6, 3, 20, 3), (44, 10, 3, 40, 8)])
def test_gpu_generate_lsc_matches_oracle(api, oracle, N, M, dim, n_obs, seed):
    import torch

    assert torch.cuda.is_available()
    sw, b = _swarm_inputs(N, M, dim, n_obs, seed)
    assert sw.n_obs == n_obs
    # a few missing neighbours (-1) and one overlapping pair exercise the zero-row and the fallback branches
    nbr = b["nbr"].astype(np.int32).copy()
    nbr[0, -1] = -1
    init = b["init"].copy()
    init[1] = init[nbr[1, 0]]  # agent 1 sits exactly on its first neighbour
    L = oracle.generate_lsc(init, nbr, sw.radius, sw.downwash, b["goal"], dim=dim)
    want = api.pack_rows(L).reshape(N, n_obs, M, 6)
    dev = torch.device("cuda", 0)
    sol = api.Solver(api.make_desc(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max))
    d_traj = torch.from_numpy(init.copy()).to(dev)
    d_nbr = torch.from_numpy(nbr).to(dev)
    d_r = torch.full((N,), sw.radius, dtype=torch.float64, device=dev)
    d_dw = torch.full((N,), sw.downwash, dtype=torch.float64, device=dev)
    d_goal = torch.from_numpy(np.ascontiguousarray(b["goal"], dtype=np.float64)).to(dev)
    d_rows = torch.full((N * n_obs * M * 6 * 4,), float("nan"), dtype=torch.float64, device=dev)
    sol.generate_lsc_device(N, n_obs, 0, d_traj, d_nbr, d_r, d_dw, d_goal, d_rows)
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy().view(api.ROW_DTYPE).reshape(N, n_obs, M, 6)
    assert (got["nx"][0, -1] == 0).all() and (got["b"][0, -1] == 0).all()  # missing neighbour -> all-zero rows
    # Same float32 staging on both sides; the fp64 enumeration differs only in operation order (1/det vs /det, FMA
    # contraction), which can move a float32 rounding by one ulp: 2e-7 on the unit normal, 2e-6 on b = d + n.p (|p| <~ 30 m)
    for f, tol in (("nx", 2e-7), ("ny", 2e-7), ("nz", 2e-7), ("b", 2e-6)):
        assert np.abs(got[f] - want[f]).max() <= tol, (f, np.abs(got[f] - want[f]).max())
    assert np.isfinite(d_rows.cpu().numpy()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 2])
def test_gpu_fallback_normal_uses_the_obstacles_current_position_on_moving_plans(api, oracle, dim):
    """Overlapping hulls on MOVING trajectories: the fallback normal is goal - obstacle POSITION (the first control point of the
    neighbour's shifted plan) for every segment (reference src/traj_planner.cpp:629-631), not goal - first point of segment m.
    With a stationary swarm (all control points equal) the two cannot be told apart; here every segment of the neighbour starts
    somewhere else."""
    import torch

    N, M, n_obs = 6, 5, 2
    rng = np.random.default_rng(17)
    init = np.zeros((N, M, 6, 3))
    for a in range(N):
        start = rng.uniform(-1, 1, 3)
        vel = rng.uniform(-1.0, 1.0, 3)
        t = (np.arange(M * 6) * 0.04).reshape(M, 6)
        init[a] = start + vel * t[..., None] + 0.02 * rng.normal(size=(M, 6, 3))
    if dim == 2:
        init[..., 2] = 1.0
    init = np.float32(init).astype(np.float64)
    nbr = np.array([[1, 2], [0, 2], [0, 1], [4, 5], [3, 5], [3, 4]], dtype=np.int32)
    init[1] = init[0] + np.float32(1e-3)   # pairs (0,1) and (3,4) overlap in every segment -> fallback everywhere
    init[4] = init[3]
    goal = np.float32(rng.uniform(-3, 3, (N, 3))).astype(np.float64)
    if dim == 2:
        goal[:, 2] = 1.0
    L = oracle.generate_lsc(init, nbr, 0.15, 2.0, goal, dim=dim)
    want = api.pack_rows(L).reshape(N, n_obs, M, 6)
    # the oracle itself: fallback direction = goal - first control point of the neighbour's plan, for the LAST segment too
    fb = goal[3] - init[4, 0, 0]
    if dim == 2:
        fb[2] = 0.0
    else:
        fb[2] /= 2.0
    fb = fb / np.linalg.norm(fb)
    nz_out = fb[2] / 2.0 if dim == 3 else 0.0
    assert np.abs(L["nrm"][3, 0, M - 1, 0] - np.array([fb[0], fb[1], nz_out])).max() <= 3e-7
    dev = torch.device("cuda", 0)
    sol = api.Solver(api.make_desc(M=M, dim=dim))
    d_rows = torch.full((N * n_obs * M * 6 * 4,), float("nan"), dtype=torch.float64, device=dev)
    sol.generate_lsc_device(N, n_obs, 0, torch.from_numpy(init.copy()).to(dev), torch.from_numpy(nbr).to(dev),
                            torch.full((N,), 0.15, dtype=torch.float64, device=dev), torch.full((N,), 2.0, dtype=torch.float64, device=dev),
                            torch.from_numpy(goal.copy()).to(dev), d_rows)
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy().view(api.ROW_DTYPE).reshape(N, n_obs, M, 6)
    for f, tol in (("nx", 2e-7), ("ny", 2e-7), ("nz", 2e-7), ("b", 2e-6)):
        assert np.abs(got[f] - want[f]).max() <= tol, (f, np.abs(got[f] - want[f]).max())


@pytest.mark.gpu
def test_gpu_generated_rows_feed_the_solver(api, oracle):
    """shift -> generate -> solve entirely on the device equals the host pipeline (rows from the oracle restatement)."""
    import torch

    N, M, dim, n_obs = 32, 5, 3, 12
    sw, b = _swarm_inputs(N, M, dim, n_obs, 5)
    dev = torch.device("cuda", 0)
    sol = api.Solver(api.make_desc(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max))
    hdr, rows, off, sfc = api.batch_from_swarm(b, sw.n_obs, M)
    r0 = sol.solve_host(hdr, rows, off, sfc)
    assert (r0["status"] == 0).all()
    sw.advance(r0["x"])
    b1 = sw.build()  # host pipeline: shift + LSC (numpy) of the next replan
    # device pipeline from the same solution
    d_x = torch.from_numpy(r0["x"].copy()).to(dev)
    d_traj = torch.zeros(N * M * 6 * 3, dtype=torch.float64, device=dev)
    sol.shift_traj_device(N, d_x, d_traj)
    torch.cuda.synchronize()
    assert np.array_equal(d_traj.cpu().numpy().reshape(N, M, 6, 3), b1["init"])  # bit-exact: float32 rounding of the same values
    d_nbr = torch.from_numpy(b1["nbr"].astype(np.int32)).to(dev)
    d_r = torch.full((N,), sw.radius, dtype=torch.float64, device=dev)
    d_dw = torch.full((N,), sw.downwash, dtype=torch.float64, device=dev)
    d_goal = torch.from_numpy(np.ascontiguousarray(b1["goal"], dtype=np.float64)).to(dev)
    d_rows = torch.zeros(N * n_obs * M * 6 * 4, dtype=torch.float64, device=dev)
    sol.generate_lsc_device(N, n_obs, 0, d_traj, d_nbr, d_r, d_dw, d_goal, d_rows)
    hdr1, rows1, off1, sfc1 = api.batch_from_swarm(b1, sw.n_obs, M)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_hdr, d_off, d_sfc = up(hdr1), up(off1), up(sfc1)
    d_xo = torch.zeros(N * sol.nv, dtype=torch.float64, device=dev)
    d_obj = torch.zeros(N, dtype=torch.float64, device=dev)
    d_st = torch.full((N,), -1, dtype=torch.int32, device=dev)
    sol.solve_device(N, n_obs, d_hdr, d_rows, d_off, d_sfc, d_xo, d_obj, d_st)
    torch.cuda.synchronize()
    r1 = sol.solve_host(hdr1, rows1, off1, sfc1)
    assert (d_st.cpu().numpy() == 0).all() and (r1["status"] == 0).all()
    # rows agree to float32 rounding (previous test) -> optima agree far inside the parity tolerances
    assert np.abs(d_xo.cpu().numpy().reshape(N, -1) - r1["x"]).max() <= 1e-5
    assert np.abs(d_obj.cpu().numpy() - r1["obj"]).max() <= 1e-6 * max(1.0, np.abs(r1["obj"]).max())


# ==================================================================================================================================
# The closest-point search pinned by constructed hulls (tests/lscgen_cases.py) and an exact referee (tests/hull_reference.py).
# Three things hold every run: the constructed result, the referee, and the oracle.  Standing bars of this kernel: 2e-7 on a normal
# component, 2e-6 on b (4e-6 under LSCQP_ROWS_F32); exactness claims are ==.
from tests import hull_reference as R  # noqa: E402
from tests import lscgen_cases as LC  # noqa: E402

from tests.lscgen_checks import (ORACLE_DEV, TOL_B, TOL_B_F32, TOL_N, _coverage_line, _dev, _exact_claims, _family_mask, _hold,  # noqa: E402
                                 _hold_device, _hold_to_referee, _masked)


def test_referee_certificate_and_recorded_gjk():
    """The referee on the un-rounded 240-hull fixture: every answer carries its certificate, and distance, point and the inside verdict
    are openGJK's, at the fixture's 1e-9 bar."""
    g = H.load_golden("gjk_hulls")
    worst = 0.0
    for c in g["cases"]:
        r = R.closest_point(c["hull"])
        assert R.certificate_holds(c["hull"], r), c["kind"]
        assert r.inside == (c["dist"] == 0.0), c["kind"]
        worst = max(worst, abs(r.dist - c["dist"]), max(abs(float(a) - b) for a, b in zip(r.point, c["closest"])))
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("dim", [3, 2])
def test_referee_confirms_every_constructed_case(dim):
    """Construction and referee agree exactly: the kind, the winning subset, and the closest point (the normal to 1e-15); every feature
    of the enumeration is the unique winner in at least four directions (3-D: 41 features at downwash 1 and at 2; 2-D: 21)."""
    cases, ref, n_ref, _ = LC.suite(dim)
    wins = {}
    for c, (kind, n, res) in zip(cases, ref):
        hull = c["rel"] * np.array([1.0, 1.0, 1.0 if dim == 3 else 0.0])
        assert R.certificate_holds(hull, res), c["name"]
        assert kind == c["kind"], (c["name"], kind)
        if c["winner"] is not None:
            assert res.subset == c["winner"], (c["name"], res.subset)
            if c["family"].startswith("feature"):
                assert res.ties == [c["winner"]], (c["name"], res.ties)  # unique: no other subset reproduces the point
                wins.setdefault((c["dwk"], c["winner"]), set()).add(tuple(c["n"]))
        if c["n"] is not None and n is not None:
            assert np.abs(n - c["n"]).max() <= 1e-15, c["name"]
    feats = LC.FEATURES_3D if dim == 3 else LC.FEATURES_2D
    for dwk in ((1, 2) if dim == 3 else (1,)):
        assert all(len(wins.get((dwk, S), ())) >= 4 for S in feats), dwk
    print("referee: %d cases, %d features x >= 4 directions x downwash %s" % (len(cases), len(feats), "1, 2" if dim == 3 else "1"))


def test_golden_hulls_nothing_left_out():
    """No golden hull sits near the float32 switch (exact distance of the rounded hull in [0.5e-5, 2e-5] m), and the referee's
    inside/outside verdict is openGJK's recorded one on every hull: none needs to be set aside."""
    hulls, dist, planar = LC.golden_hulls()
    assert len(hulls) == 3240 and planar.sum() >= 40
    for dim in (3, 2):
        cases, ref, _, _ = LC.golden_suite(dim)
        d = np.array([r[2].dist for r in ref])
        assert not ((d >= 0.5e-5) & (d <= 2e-5)).any(), d[(d >= 0.5e-5) & (d <= 2e-5)]
        assert not any(r[0] == "near" for r in ref)
        if dim == 3:
            assert np.array_equal(d == 0.0, dist == 0.0), np.nonzero((d == 0.0) != (dist == 0.0))[0]
            assert d[d > 0].min() > 3e-4  # the smallest positive distance of the fixtures: 3.2e-4 m


@pytest.mark.parametrize("dim,mode", [(3, "lsc"), (3, "clsc"), (2, "lsc"), (2, "clsc")])
def test_oracle_pairs_against_constructed_results_and_referee(oracle, api, dim, mode):
    cases, _, n_ref, n_con = LC.suite(dim)
    M = 5
    pk = LC.pack_pairs(cases, M, dim, hull_segments=M if mode == "lsc" else M - 1, z_noise=(dim == 2 and mode == "lsc"))
    got = LC.oracle_pairs(oracle, api, 0 if mode == "lsc" else 1, pk)
    _hold(got, LC.expected_for_pack(cases, pk, n_con, mode), what="oracle %s %d-D vs constructed" % (mode, dim))
    _hold(got, LC.expected_for_pack(cases, pk, n_ref, mode), what="oracle %s %d-D vs referee" % (mode, dim))
    _exact_claims(cases, pk, got, mode)
    if mode == "lsc":  # (M = 2 on the same cases: the other segment count the families are packed at)
        pk2 = LC.pack_pairs(cases, 2, dim, z_noise=dim == 2)
        _hold(LC.oracle_pairs(oracle, api, 0, pk2), LC.expected_for_pack(cases, pk2, n_con, mode), what="oracle lsc %d-D M=2" % dim)


@pytest.mark.parametrize("dim,tall", [(3, False), (2, False), (3, True)])
def test_oracle_obstacles_against_constructed_results(oracle, api, dim, tall):
    cases, _, n_ref, n_con = LC.suite(2 if tall else dim)
    pk = LC.pack_obstacles(cases, 5, dim, tall=tall)
    got = LC.oracle_obstacles(oracle, api, pk)
    _hold(got, LC.expected_for_obstacles(cases, pk, n_con), what="oracle obstacles %d-D tall=%s vs constructed" % (dim, tall))
    _hold(got, LC.expected_for_obstacles(cases, pk, n_ref), what="oracle obstacles %d-D tall=%s vs referee" % (dim, tall))
    _exact_claims(cases, pk, got, "obstacle")
    if tall:  # planar separation: nz is 0 unless the fallback (goal - position, z / downwash) speaks
        hullish = np.array([[ci >= 0 and cases[ci]["kind"] == "hull" for ci in row] for row in pk["slot"]])
        assert (got[hullish][..., 2] == 0).all()


@pytest.mark.parametrize("dim", [3, 2])
def test_oracle_against_referee_on_golden_hulls(oracle, api, dim):
    """The float32-rounded golden hulls (3-D: all 3240 through the exact route of the referee; 2-D: the xy projections of the planar
    ones) through generate_lsc: the normals and b against the referee's c / |c|.  This is where ORACLE_DEV is measured."""
    cases, _, n_ref, _ = LC.golden_suite(dim)
    pk = LC.pack_pairs(cases, 5, dim)
    got = LC.oracle_pairs(oracle, api, 0, pk)
    dn, db = _dev(got, LC.expected_for_pack(cases, pk, n_ref, "lsc"))
    print("oracle vs referee, golden %d-D (%d hulls): normal %.3g  b %.3g" % (dim, len(cases), dn, db))
    assert dn <= ORACLE_DEV["golden%dd" % dim][0] and db <= ORACLE_DEV["golden%dd" % dim][1], (dn, db)


def test_oracle_against_referee_on_slivers(oracle, api):
    """the sliver family in every packing the device tests use (b = d + n . p_obs depends on the neighbour's points): the worst is ORACLE_DEV"""
    cases, _, n_ref, _ = LC.suite(3)
    dn = db = 0.0
    for mode, M in (("lsc", 5), ("lsc", 2), ("clsc", 5), ("clsc", 2)):
        pk = LC.pack_pairs(cases, M, 3, hull_segments=M if mode == "lsc" else M - 1)
        got = LC.oracle_pairs(oracle, api, 0 if mode == "lsc" else 1, pk)
        d = _dev(got, _masked(LC.expected_for_pack(cases, pk, n_ref, mode), _family_mask(cases, pk, ("sliver",))))
        dn, db = max(dn, d[0]), max(db, d[1])
    pk = LC.pack_obstacles(cases, 5, 3)
    d = _dev(LC.oracle_obstacles(oracle, api, pk), _masked(LC.expected_for_obstacles(cases, pk, n_ref), _family_mask(cases, pk, ("sliver",))))
    dn, db = max(dn, d[0]), max(db, d[1])
    print("oracle vs referee, slivers: normal %.3g  b %.3g" % (dn, db))
    assert dn <= ORACLE_DEV["sliver"][0] and db <= ORACLE_DEV["sliver"][1], (dn, db)


# ---- the same families on the device -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim,entry,M,rows_f32", [(3, "lsc", 5, False), (3, "constraints", 5, False), (3, "lsc", 2, False),
                                                  (2, "lsc", 5, False), (2, "constraints", 2, False), (3, "constraints", 5, True)])
def test_gpu_generate_lsc_on_constructed_hulls(api, oracle, dim, entry, M, rows_f32):
    """generate_lsc_kernel<LSC> on every constructed family (feature coverage at downwash 1 and 2, degenerate shapes, slivers, the
    1e-5f switch, the inside test, fallback rows), one hull per (agent, segment), in one launch."""
    cases, _, n_ref, n_con = LC.suite(dim)
    pk = LC.pack_pairs(cases, M, dim, z_noise=dim == 2)
    got = LC.run_pairs_device(api, api.GEN_LSC, pk, entry=entry, rows_f32=rows_f32)
    _hold_device(cases, pk, got, LC.oracle_pairs(oracle, api, 0, pk), n_con, n_ref, "lsc",
                 lambda n: LC.expected_for_pack(cases, pk, n, "lsc"), rows_f32)
    _coverage_line(cases, pk, dim, "generate_lsc (%s, M=%d)" % (entry, M))


@pytest.mark.gpu
@pytest.mark.parametrize("dim,tall,rows_f32", [(3, False, False), (2, False, False), (3, True, False), (3, False, True)])
def test_gpu_obstacle_generator_on_constructed_hulls(api, oracle, dim, tall, rows_f32):
    """generate_lsc_obstacle_kernel with a static obstacle per agent (velocity 0, size prediction off: d = radius + r_own), and with a
    tall type-0 obstacle (downwash above the threshold) whose answer is the projected 2-D case."""
    cases, _, n_ref, n_con = LC.suite(2 if tall else dim)
    pk = LC.pack_obstacles(cases, 5, dim, tall=tall)
    got = LC.run_obstacles_device(api, pk, rows_f32=rows_f32)
    _hold_device(cases, pk, got, LC.oracle_obstacles(oracle, api, pk), n_con, n_ref, "obstacle",
                 lambda n: LC.expected_for_obstacles(cases, pk, n), rows_f32)
    if tall:
        hullish = np.array([[ci >= 0 and cases[ci]["kind"] == "hull" for ci in row] for row in pk["slot"]])
        assert (got[hullish][..., 2] == 0).all()
    _coverage_line(cases, pk, 2 if tall else dim, "obstacle generator (tall=%s)" % tall)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 2])
def test_gpu_generate_lsc_on_the_golden_hulls(api, oracle, dim):
    """All 3240 recorded openGJK hulls (float32-rounded) through the LSC kernel in one launch, and the xy projections of the planar
    ones through the 2-D path: against the exact referee at the measured bar, and against the oracle at the standing bars."""
    cases, _, n_ref, _ = LC.golden_suite(dim)
    pk = LC.pack_pairs(cases, 5, dim)
    got = LC.run_pairs_device(api, api.GEN_LSC, pk, entry="lsc")
    _hold_to_referee(got, LC.expected_for_pack(cases, pk, n_ref, "lsc"), "golden%dd" % dim, what="device vs referee, golden %d-D" % dim)
    _hold(got, LC.oracle_pairs(oracle, api, 0, pk), what="device vs oracle, golden %d-D" % dim)


def _raw_generate(api, mode, M, dim, n_agents, n_obs, first, t, rows_f32, n_obs_total, slot0, d_rows):
    """lscqp_generate_lsc_raw_ (library-internal): the launch itself, for shapes the handle does not admit (M = 1)"""
    import ctypes as C

    import torch

    fn = api.lib().lscqp_generate_lsc_raw_
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int32, C.c_int64] + [C.c_void_p] * 7 + [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    rc = fn(mode, M, dim, n_agents, n_obs, first, p(t["traj"]), None, p(t["nbr"]), p(t["radius"]), p(t["downwash"]), p(t["goal"]), p(t.get("goal_all")),
            int(rows_f32), n_obs_total, slot0, p(d_rows), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("n_units,first", [(1, 0), (255, 0), (256, 3), (257, 0), (513, 5)])
def test_gpu_generate_lsc_launch_shapes(api, oracle, n_units, first):
    """n_units on both sides of the 256-thread block (one unit per agent: M = 1, n_obs = 1), a missing neighbour (-1) in the first and
    in the last unit of a block, first_agent > 0; the row buffer is pre-filled and holds exactly n_units * 6 rows plus a guard."""
    import torch

    cases, _, _, n_con = LC.suite(3)
    pick = [i for i, c in enumerate(cases) if c["family"] != "sliver"]
    sub = [cases[pick[(7 * k) % len(pick)]] for k in range(n_units)]
    nrm = [n_con[pick[(7 * k) % len(pick)]] for k in range(n_units)]
    pk = LC.pack_pairs(sub, 1, 3, seed=n_units)
    assert pk["N"] == n_units
    order = pk["slot"][:, 0]  # pack_pairs groups by downwash: the case in unit a
    want = LC.expected_for_pack(sub, pk, nrm, "lsc").reshape(n_units, 6, 4)
    missing = sorted({u for u in (0, 255, 256, 511, n_units - 1) if u < n_units and n_units > 1})
    nbr = pk["nbr"].copy() + first
    nbr[missing] = -1
    want[missing] = 0.0
    pad = lambda a: np.concatenate([np.zeros((first,) + a.shape[1:], a.dtype), a])  # noqa: E731
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t = dict(traj=up(pad(pk["traj"])), nbr=up(nbr), radius=up(pad(pk["radius"]) + (pad(pk["radius"]) == 0)), downwash=up(pad(pk["downwash"]) + (pad(pk["downwash"]) == 0)),
             goal=up(pk["goal_all"][:n_units]))
    guard = 64
    d_rows = torch.full(((n_units * 6 + guard) * 32,), 0xFF, dtype=torch.uint8, device=dev)
    _raw_generate(api, 0, 1, 3, n_units, 1, first, t, False, 1, 0, d_rows)
    buf = d_rows.cpu().numpy()
    got = LC.rows_array(buf[: n_units * 6 * 32], api, False, (n_units, 6))
    assert (buf[n_units * 6 * 32:] == 0xFF).all()  # nothing past the last unit
    assert (got[missing] == 0).all()
    _hold(got, want, what="launch shape n_units=%d first=%d" % (n_units, first))
    assert len(order) == n_units


@pytest.mark.gpu
@pytest.mark.parametrize("rows_f32", [False, True])
@pytest.mark.parametrize("slot0", [0, 1, 3])
def test_gpu_remapped_store_leaves_every_other_slot_untouched(api, oracle, slot0, rows_f32):
    """n_obs = 2 neighbour slots written into an agent's block of n_obs_total = 5 slots at slot0 = 0, in the middle and at the end, over
    several 256-thread blocks, in fp64 rows and in LSCQP_ROWS_F32: the owned slots hold the rows, and EVERY byte of every slot not
    owned is still the sentinel."""
    import torch

    cases, _, _, n_con = LC.suite(3)
    M, n_obs, n_tot = 5, 2, 5
    pk = LC.pack_pairs(cases, M, 3)
    N = pk["N"]
    assert N * n_obs * M > 3 * 256
    # second slot: the partner of the next agent (not a constructed hull: held to the oracle), with a missing neighbour here and there
    nbr = np.stack([pk["nbr"][:, 0], np.roll(pk["nbr"][:, 0], -1)], axis=1).astype(np.int32)
    nbr[::7, 1] = -1
    L = oracle.generate_lsc(pk["traj"], nbr, pk["radius"], pk["downwash"], pk["goal_all"][:N], dim=3)
    r = api.pack_rows(L).reshape(N, n_obs, M, 6)
    want_oracle = np.stack([r["nx"], r["ny"], r["nz"], r["b"]], axis=-1)
    dev = torch.device("cuda", 0)
    kw = dict(row_format=api.ROWS_F32) if rows_f32 else {}
    sol = api.Solver(api.make_desc(M=M, dim=3, world_min=(-40, -40, -40), world_max=(40, 40, 40), **kw))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    item = 16 if rows_f32 else 32
    d_rows = torch.full((N * n_tot * M * 6 * item,), 0xFF, dtype=torch.uint8, device=dev)
    sol.generate_constraints_device_ex(api.GEN_LSC, N, n_obs, 0, up(pk["traj"]), up(nbr), up(pk["radius"]), up(pk["downwash"]), up(pk["goal_all"]),
                                       d_rows, n_tot, slot0)
    torch.cuda.synchronize()
    buf = d_rows.cpu().numpy().reshape(N, n_tot, M * 6 * item)
    owned = np.zeros(n_tot, dtype=bool)
    owned[slot0:slot0 + n_obs] = True
    assert (buf[:, ~owned] == 0xFF).all(), np.argwhere(buf[:, ~owned] != 0xFF)[:4]
    got = LC.rows_array(np.ascontiguousarray(buf[:, owned]).reshape(-1), api, rows_f32, (N, n_obs, M, 6))
    tol_b = TOL_B_F32 if rows_f32 else TOL_B
    _hold(got, want_oracle, TOL_N, tol_b, what="remap slot0=%d vs oracle" % slot0)
    rest = _family_mask(cases, pk, ("sliver",), keep=False)
    _hold(got[:, 0], _masked(LC.expected_for_pack(cases, pk, n_con, "lsc"), rest), TOL_N, tol_b, what="remap slot0=%d vs constructed" % slot0)
    assert (got[::7, 1] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rows_f32", [False, True])
def test_gpu_obstacle_remapped_store_leaves_every_other_slot_untouched(api, oracle, rows_f32):
    """the obstacle generator's own remap (row0 from n_obs_total and slot0): slot 1 of 3, sentinels everywhere else"""
    import torch

    cases, _, _, n_con = LC.suite(3)
    pk = LC.pack_obstacles(cases, 5, 3)
    N, M, n_tot, slot0 = pk["N"], 5, 3, 1
    dev = torch.device("cuda", 0)
    kw = dict(row_format=api.ROWS_F32) if rows_f32 else {}
    sol = api.Solver(api.make_desc(M=M, dim=3, world_min=(-40, -40, -40), world_max=(40, 40, 40), **kw))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    hdr = np.zeros(N, api.HEADER_DTYPE)
    hdr["amax"] = 2.0
    table = np.zeros(N, api.OBSTACLE_DTYPE)
    for f in ("position", "velocity", "radius", "downwash", "max_acc", "type"):
        table[f] = pk["table"][f]
    item = 16 if rows_f32 else 32
    d_rows = torch.full((N * n_tot * M * 6 * item,), 0xFF, dtype=torch.uint8, device=dev)
    sol.generate_lsc_obstacles_device(LC.obstacle_param(api), N, 1, 0, up(pk["traj"]), up(pk["ids"]), up(table), up(pk["radius"]), up(pk["goal"]),
                                      up(hdr), d_rows, n_tot, slot0)
    torch.cuda.synchronize()
    buf = d_rows.cpu().numpy().reshape(N, n_tot, M * 6 * item)
    assert (buf[:, [0, 2]] == 0xFF).all()
    got = LC.rows_array(np.ascontiguousarray(buf[:, 1]).reshape(-1), api, rows_f32, (N, M, 6))
    rest = _family_mask(cases, pk, ("sliver",), keep=False)
    _hold(got, _masked(LC.expected_for_obstacles(cases, pk, n_con), rest), TOL_N, TOL_B_F32 if rows_f32 else TOL_B, what="obstacle remap vs constructed")
