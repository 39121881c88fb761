"""The run-time-shaped kernel (csrc/lscqp_generic.hip): every (M, dim, planner mode) the reference accepts and neighbour counts beyond
the compiled instances' register slots -- the reference builds its QP for whatever param.M / getObsSize() are
(src/traj_optimizer.cpp:4-16, 399-437; src/param.cpp:71, 128-163).  Parity against the CPU oracle at the bar of test_gpu_parity.py.

Every case that is about this kernel proves that this kernel answered (`_kernel_of`): Solver.instance_work() selects through the same
find_instance() call, with the same switches, as the launch, and fails with ERR_UNSUPPORTED ("... carries no instruction counts") exactly
when that call finds no compiled instance -- which is when the launch goes to the run-time-shaped kernel."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

OBJ_TOL, KKT_TOL, X_TOL = 1e-8, 1e-8, H.PathTol()  # x: 1e-8 m for the dual active-set phase, 1e-6 m for the interior-point kernel
COMPILED_ES1 = {(5, 3), (6, 3), (7, 3), (4, 3), (3, 3), (2, 3), (10, 2), (8, 2), (5, 2), (10, 3)}
COMPILED_ES0 = {(5, 3), (5, 2), (10, 2)}
LDS_PER_CU = 160 * 1024  # gfx950 (csrc/lscqp_launch.hpp: kMaxLdsBytes)
RAGGED_K = (0, 1, 3, 8, 0, 5, 2, 8, 4, 7, 6, 0)  # neighbours kept per instance of the ragged batches (N = 12, n_obs = 8)


def _mode(api, lsc_mode):
    return api.PLANNER_LSC if lsc_mode else api.PLANNER_DLSC


def _kernel_of(api, n, n_obs, **desc):
    """"generic" or "compiled": the kernel a launch of n instances with n_obs_max = n_obs goes to, for a handle made NOW from this
    description (the switches a handle reads when it is created -- LSCQP_FORCE_GENERIC -- included).  The selection is a function of
    (switches, M, dim, end stop, precision, n_obs_max, n, CU count) alone, so a second handle of the same description made under the
    same environment launches what this one reports."""
    sol = api.Solver(api.make_desc(**desc))
    try:
        w = sol.instance_work(n, n_obs)
    except api.LscqpError as e:
        assert e.code == api.ERR_UNSUPPORTED and "run-time-shaped kernel carries no instruction counts" in str(e), e
        return "generic"
    assert w["kernel"].startswith("lscqp_pdip_kernel<%d,%d," % (desc.get("M", 5), desc.get("dim", 3))), w["kernel"]
    return "compiled"


def _force(monkeypatch, forced):
    monkeypatch.delenv("LSCQP_FORCE_GENERIC", raising=False)
    if forced:
        monkeypatch.setenv("LSCQP_FORCE_GENERIC", "1")


def test_every_shape_the_reference_accepts_has_a_kernel(api):
    """No device needed: lscqp_create succeeds for every (2 <= M <= 12, dim 2 | 3, planner mode) -- compiled instance or the run-time-shaped
    kernel -- and states a neighbour capacity; only M > 12 is refused."""
    for M in range(2, 13):
        for dim in (2, 3):
            for mode in (api.PLANNER_LSC, api.PLANNER_DLSC, api.PLANNER_BVC, api.PLANNER_RSFC):
                s = api.Solver(api.make_desc(M=M, dim=dim, planner_mode=mode))
                cap = s.max_obstacles()
                assert cap >= 40, (M, dim, mode, cap)
                if M <= 6:
                    assert cap >= 64, (M, dim, mode, cap)
    with pytest.raises(api.LscqpError):
        api.Solver(api.make_desc(M=13, dim=3))


def test_the_selection_probe_honours_the_force_switch(api, monkeypatch):
    """No device needed.  What `_kernel_of` reports follows the switch, through the environment and through Solver.set_knob alike: every
    (M <= 10, dim, end stop) has a compiled instance for 4 neighbours and leaves it when forced; M = 11, 12 have none either way."""
    for forced in (False, True):
        _force(monkeypatch, forced)
        for M in range(2, 13):
            for dim in (2, 3):
                for lsc_mode in (True, False):
                    want = "generic" if (forced or M > 10) else "compiled"
                    assert _kernel_of(api, 8, 4, M=M, dim=dim, planner_mode=_mode(api, lsc_mode)) == want, (forced, M, dim, lsc_mode)
    _force(monkeypatch, False)
    sol = api.Solver(api.make_desc(M=5, dim=3))
    assert sol.instance_work(8, 4)["max_obstacles"] >= 4
    sol.set_knob("force_generic", 1)
    with pytest.raises(api.LscqpError) as e:
        sol.instance_work(8, 4)
    assert e.value.code == api.ERR_UNSUPPORTED
    sol.set_knob("force_generic", 0)
    assert sol.instance_work(8, 4)["max_obstacles"] >= 4
    # beyond the register slots of the largest compiled instance the launch falls through without the switch
    assert _kernel_of(api, 80, 64, M=10, dim=3) == "generic" and _kernel_of(api, 80, 30, M=9, dim=3) == "compiled"


def test_the_lds_carve_of_the_largest_shape_ends_at_the_capacity(api):
    """No device needed: at M = 12 in 3-D, with and without the end stop, the carve for `max_obstacles()` neighbours fits the CU's 160 KB and
    the carve for one more does not.  NOTES.md section 4 states the figures: 55 without the end stop (nz = 108), 60 with it (nz = 102: a
    smaller triangle)."""
    L = api.lib()
    L.lscqp_generic_lds_bytes.restype, L.lscqp_generic_lds_bytes.argtypes = C.c_size_t, [C.c_int] * 4
    L.lscqp_generic_max_obstacles.restype, L.lscqp_generic_max_obstacles.argtypes = C.c_int, [C.c_int] * 3
    for es, mode in ((1, api.PLANNER_LSC), (0, api.PLANNER_DLSC)):
        cap = api.Solver(api.make_desc(M=12, dim=3, planner_mode=mode)).max_obstacles()
        assert cap == L.lscqp_generic_max_obstacles(12, 3, es) == (60 if es else 55), (es, cap)
        assert L.lscqp_generic_lds_bytes(12, 3, es, cap) <= LDS_PER_CU < L.lscqp_generic_lds_bytes(12, 3, es, cap + 1), (es, cap)


def _swarm_vs_oracle(api, oracle, M, dim, n_obs, lsc_mode, N=8, steps=2, seed=3, warm=True):
    from lsc_dr_planner_amd import synth

    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=seed)
    cls = oracle.make_class(M=M, dim=dim, planner_lsc=lsc_mode, use_sfc=True, world_min=sw.world_min, world_max=sw.world_max)
    sol = api.Solver(api.make_desc(M=M, dim=dim, planner_mode=api.PLANNER_LSC if lsc_mode else api.PLANNER_DLSC,
                                   world_min=sw.world_min, world_max=sw.world_max))
    worst = (0.0, 0.0)
    for step in range(steps):
        b = sw.build()
        ag, lsc, off, sfc = H.swarm_oracle_inputs(oracle, sw, b)
        R = oracle.solve_batch(cls, ag, lsc, off, sfc, threads=8)
        hdr, rows, roff, sfcp = api.batch_from_swarm(b, sw.n_obs, M)
        hdr["terminal_segments"] = [oracle.terminal_segments(cls, ag[q:q + 1]) for q in range(N)]
        G = sol.solve_host(hdr, rows, roff, sfcp, x_init=api.x_init_from_swarm(b, dim) if (warm and step > 0) else None)
        assert (R["status"] == 0).all() and (G["status"] == 0).all(), (M, dim, lsc_mode, step, G["status"], R["status"])
        dx = np.abs(G["x"] - R["x"]).max()
        do = (np.abs(G["obj"] - R["obj"]) / np.maximum(1.0, np.abs(R["obj"]))).max()
        assert dx <= X_TOL and do <= OBJ_TOL, (M, dim, lsc_mode, step, dx, do)
        q = step % N
        stat, eqv, iqv = H.kkt_from_primal(oracle, cls, ag[q:q + 1], np.ascontiguousarray(b["lsc"][q]), np.ascontiguousarray(b["sfc"][q]), G["x"][q])
        assert stat <= KKT_TOL and eqv <= KKT_TOL and iqv <= KKT_TOL, (M, dim, lsc_mode, step, stat, eqv, iqv)
        worst = (max(worst[0], dx), max(worst[1], do))
        sw.advance(G["x"])
    return worst, G


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True], ids=["as_selected", "run_time_shaped_kernel"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("lsc_mode", [True, False])
def test_full_shape_grid_against_the_oracle(api, oracle, torch_cuda, monkeypatch, dim, lsc_mode, forced):
    """The full (M, dim, end stop) grid, 2 <= M <= 12, 4 neighbours per agent.  As selected, every shape with M <= 10 runs on its compiled
    instance and M = 11, 12 -- which have none -- on the run-time-shaped kernel; forced, that kernel answers on every shape of the grid.
    Either way the kernel named meets the oracle at the stated bar (cold first replan, warm-started second), OPTIMAL on both sides."""
    _force(monkeypatch, forced)
    for M in range(2, 13):
        want = "generic" if (forced or M > 10) else "compiled"
        assert _kernel_of(api, 8, 4, M=M, dim=dim, planner_mode=_mode(api, lsc_mode)) == want, (M, dim, lsc_mode, forced)
        _swarm_vs_oracle(api, oracle, M, dim, n_obs=4, lsc_mode=lsc_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("M,dim,n_obs,lsc_mode", [(5, 3, 20, True), (10, 2, 9, True), (6, 3, 12, True), (10, 3, 24, True), (5, 3, 10, False), (3, 3, 6, True),
                                                  (10, 3, 12, False), (9, 3, 12, False), (8, 3, 8, True), (2, 2, 2, True)])
def test_generic_kernel_on_shapes_with_compiled_instances(api, oracle, torch_cuda, monkeypatch, M, dim, n_obs, lsc_mode):
    """LSCQP_FORCE_GENERIC=1: the run-time-shaped kernel on the shapes every other fixture of the suite exists for -- it has to meet
    the oracle where the compiled instances do, and the two kernels agree with each other far inside the bar.  Beyond the end-stop class:
    DLSC at nz = 90 and 81 (the end-stop-free branch of the index helpers with more rows than one wavefront has lanes), nz = 66 (two rows
    in the substitution's second register) and the smallest system there is, nz = 8."""
    _force(monkeypatch, False)
    assert _kernel_of(api, 12, n_obs, M=M, dim=dim, planner_mode=_mode(api, lsc_mode)) == "compiled"
    _, G_fast = _swarm_vs_oracle(api, oracle, M, dim, n_obs, lsc_mode, N=12, steps=3, seed=7)
    _force(monkeypatch, True)
    assert _kernel_of(api, 12, n_obs, M=M, dim=dim, planner_mode=_mode(api, lsc_mode)) == "generic"
    _, G_gen = _swarm_vs_oracle(api, oracle, M, dim, n_obs, lsc_mode, N=12, steps=3, seed=7)
    assert np.abs(G_fast["x"] - G_gen["x"]).max() <= 2e-7
    assert (np.abs(G_fast["obj"] - G_gen["obj"]) / np.maximum(1.0, np.abs(G_fast["obj"]))).max() <= 1e-9
    # bitwise reproducible: no atomics, fixed reduction orders
    _, G_gen2 = _swarm_vs_oracle(api, oracle, M, dim, n_obs, lsc_mode, N=12, steps=3, seed=7)
    assert np.array_equal(G_gen["x"], G_gen2["x"]) and np.array_equal(G_gen["obj"], G_gen2["obj"])


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True], ids=["as_selected", "run_time_shaped_kernel"])
@pytest.mark.parametrize("M,dim,n_obs", [(5, 3, 64), (5, 3, 100), (6, 3, 64), (10, 2, 64), (10, 3, 64), (9, 3, 30)])
def test_more_neighbours_than_the_two_wavefront_instances_hold(api, oracle, torch_cuda, monkeypatch, M, dim, n_obs, forced):
    """64 (100) neighbours per agent: beyond the 48 / 40 of round 2's largest compiled instances (every obstacle gets its rows in the
    reference, src/traj_optimizer.cpp:399-437).  As selected, the launch goes to a four-wavefront compiled instance where one holds the
    count (M = 5: 72 / 108, M = 6: 56, M = 9: 40) and falls through to the run-time-shaped kernel otherwise; forced, it is that kernel in
    every case -- OPTIMAL at the oracle's optimum either way, never CAPACITY."""
    monkeypatch.delenv("LSCQP_FORCE_GENERIC", raising=False)
    if forced:
        monkeypatch.setenv("LSCQP_FORCE_GENERIC", "1")
    sol = api.Solver(api.make_desc(M=M, dim=dim))
    assert sol.max_obstacles() >= n_obs
    _swarm_vs_oracle(api, oracle, M, dim, n_obs, True, N=max(80, n_obs + 8), steps=2, seed=13)


# ---- planner modes -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("M,forced", [(5, True), (11, False)], ids=["M5_forced", "M11"])
def test_rsfc_relaxes_the_z_bounds_of_the_first_segment_on_the_run_time_shaped_kernel(api, oracle, torch_cuda, monkeypatch, M, forced):
    """test_gpu_parity.py::test_rsfc_planner_mode_relaxes_the_z_bounds_of_the_first_segment on this kernel (the +-100 m z interval of
    segment 0, reference src/traj_optimizer.cpp:255-258): an agent just under the world ceiling, climbing and braking at the limit, has to
    overshoot the ceiling in its first segment.  With the world box on segment 0 (DLSC) the ceiling binds and the QP has no point, on both
    sides; in RSFC mode it does not bind there, and kernel and oracle agree on the optimum."""
    dim = 3
    wmin, wmax = [-5, -5, 0], [5, 5, 2.5]
    _force(monkeypatch, forced)
    ag = oracle.make_agent(p0=[0, 0, 2.495], v0=[0, 0, 0.18], a0=[0, 0, -1.9], goal=[0.5, 0, 2.0], next_waypoint=[0.5, 0, 2.0])
    for name, mode_abi, mode_orc in (("dlsc", api.PLANNER_DLSC, 0), ("rsfc", api.PLANNER_RSFC, 2)):
        desc = dict(M=M, dim=dim, planner_mode=mode_abi, use_sfc=False, world_min=wmin, world_max=wmax)
        assert _kernel_of(api, 1, 0, **desc) == "generic"
        sol = api.Solver(api.make_desc(**desc))
        cls = oracle.make_class(M=M, dim=dim, planner_lsc=mode_orc, use_sfc=False, world_min=wmin, world_max=wmax)
        hdr, rows, off, sfc = H.abi_batch(api, oracle, cls, [ag], [None], None, M)
        G = sol.solve_host(hdr, None, None, None)
        o = oracle.solve(cls, ag, None, None)
        if name == "dlsc":
            assert G["status"][0] != 0 and o["status"] != 0
            continue
        assert G["status"][0] == 0 and o["status"] == 0
        assert abs(o["obj"] - G["obj"][0]) <= OBJ_TOL * max(1.0, abs(o["obj"])) and np.abs(o["x"] - G["x"][0]).max() <= X_TOL
        z = G["x"][0].reshape(dim, M, 6)[2]
        assert z[0, 3:].max() > 2.5 + 1e-3 and z[1:].max() <= 2.5 + 1e-9  # segment 0 overshoots, later segments keep the world box


def _solve_device(api, torch, sol, hdr, rows, off, sfc, n_obs_max):
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    n = len(hdr)
    d_x = torch.zeros(n * sol.nv, dtype=torch.float64, device=dev)
    d_obj = torch.zeros(n, dtype=torch.float64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_info = torch.zeros(n * api.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_rows = rows if isinstance(rows, torch.Tensor) else up(rows)
    sol.solve_device(n, n_obs_max, up(hdr), d_rows, up(off), up(sfc), d_x, d_obj, d_st, d_info)
    torch.cuda.synchronize()
    return dict(x=d_x.cpu().numpy().reshape(n, sol.nv), obj=d_obj.cpu().numpy(), status=d_st.cpu().numpy(),
                info=d_info.cpu().numpy().view(api.INFO_DTYPE))


@pytest.mark.gpu
def test_bvc_mode_end_to_end_at_the_longest_horizon(api, oracle, torch_cuda):
    """test_lscmode.py::test_bvc_mode_end_to_end_on_the_default_shape at M = 12 in 3-D (nz = 108, the largest reduced system): generateBVC
    rows from the device feed the QP without the LSC-mode end-stop rows; the oracle re-solves from the same rows."""
    from lsc_dr_planner_amd import synth

    torch = torch_cuda
    N, M, dim, n_obs = 10, 12, 3, 9
    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=2)
    b = sw.build()
    dev = torch.device("cuda", 0)
    desc = dict(M=M, dim=dim, planner_mode=api.PLANNER_BVC, world_min=sw.world_min, world_max=sw.world_max)
    assert _kernel_of(api, N, n_obs, **desc) == "generic"
    sol = api.Solver(api.make_desc(**desc))
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True, planner_lsc=False, world_min=sw.world_min, world_max=sw.world_max)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_rows = torch.zeros(N * n_obs * M * 6 * 4, dtype=torch.float64, device=dev)
    sol.generate_constraints_device(api.GEN_BVC, N, n_obs, 0, up(b["init"]), up(b["nbr"].astype(np.int32)), up(np.full(N, sw.radius)),
                                    up(np.full(N, sw.downwash)), up(np.ascontiguousarray(b["goal"], dtype=np.float64)), d_rows)
    hdr, _, off, sfc = api.batch_from_swarm(b, sw.n_obs, M)
    G = _solve_device(api, torch, sol, hdr, d_rows, off, sfc, n_obs)
    R = d_rows.cpu().numpy().view(api.ROW_DTYPE).reshape(N, n_obs, M, 6)
    assert (G["status"] == 0).all(), G["status"]
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
        assert abs(o["obj"] - G["obj"][q]) <= OBJ_TOL * max(1.0, abs(o["obj"])) and np.abs(o["x"] - G["x"][q]).max() <= X_TOL, q
    # no end stop in BVC mode: some plan still moves at the end of the horizon
    X = G["x"].reshape(N, dim, M, 6)
    assert np.abs(X[:, :, M - 1, 5] - X[:, :, M - 1, 4]).max() > 1e-4


# ---- ragged batches ------------------------------------------------------------------------------------------------------------------------


def _ragged(api, oracle, M, dim, lsc_mode, ks, n_obs=8, seed=7):
    """One cold replan of a 12-agent swarm in which instance q keeps its first ks[q] neighbours (the [obstacle][segment][point] row block
    of an instance, cut after ks[q] obstacles, is the ABI layout of an instance with that many).  -> (swarm, oracle class, ABI arrays,
    oracle arrays)."""
    from lsc_dr_planner_amd import synth

    N, P = len(ks), 6 * M
    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=seed)
    assert sw.n_obs == n_obs
    cls = oracle.make_class(M=M, dim=dim, planner_lsc=lsc_mode, use_sfc=True, world_min=sw.world_min, world_max=sw.world_max)
    b = sw.build()
    ag, lsc, _, sfc_o = H.swarm_oracle_inputs(oracle, sw, b)
    hdr, rows, _, sfc = api.batch_from_swarm(b, n_obs, M)
    ks = np.asarray(ks, dtype=np.int32)
    ag["n_obs"], hdr["n_obs"] = ks, ks
    hdr["terminal_segments"] = [oracle.terminal_segments(cls, ag[q:q + 1]) for q in range(N)]
    off = np.concatenate([[0], np.cumsum(ks.astype(np.int64) * P)]).astype(np.uint64)
    rows_r = np.concatenate([rows.reshape(N, n_obs * P)[q, :ks[q] * P] for q in range(N)])
    lsc_r = np.concatenate([lsc.reshape(N, n_obs * P)[q, :ks[q] * P] for q in range(N)])
    return sw, cls, (hdr, rows_r, off, sfc), (ag, lsc_r, off[:-1].astype(np.int64), sfc_o)


@pytest.mark.gpu
@pytest.mark.parametrize("M,dim,lsc_mode,forced", [(12, 3, False, False), (5, 3, True, True)], ids=["M12_dlsc", "M5_lsc_forced"])
def test_ragged_batch_on_the_run_time_shaped_kernel(api, oracle, torch_cuda, monkeypatch, M, dim, lsc_mode, forced):
    """One batch whose instances have 0 .. 8 neighbours each (n_obs_max = 8): every instance meets the oracle built with its own count, and
    its x, objective and status are bit for bit what a batch of ONE with n_obs_max = its count returns -- nothing in the kernel's arithmetic
    depends on n_obs_max (only the LDS carve behind the matrix does) or on the instance's place in the batch."""
    _force(monkeypatch, forced)
    P = 6 * M
    sw, cls, (hdr, rows, off, sfc), (ag, lsc, loff, sfc_o) = _ragged(api, oracle, M, dim, lsc_mode, RAGGED_K)
    N = len(hdr)
    desc = dict(M=M, dim=dim, planner_mode=_mode(api, lsc_mode), world_min=sw.world_min, world_max=sw.world_max)
    assert _kernel_of(api, N, max(RAGGED_K), **desc) == "generic"
    sol = api.Solver(api.make_desc(**desc))
    G = sol.solve_host(hdr, rows, off, sfc)
    R = oracle.solve_batch(cls, ag, lsc, loff, sfc_o, threads=8)
    assert (R["status"] == 0).all() and (G["status"] == 0).all(), (G["status"], R["status"])
    dx = np.abs(G["x"] - R["x"]).max(axis=1)
    do = np.abs(G["obj"] - R["obj"]) / np.maximum(1.0, np.abs(R["obj"]))
    print("ragged (%d, %d): max |dx| %.3g, max rel dobj %.3g" % (M, dim, dx.max(), do.max()))
    assert dx.max() <= X_TOL and do.max() <= OBJ_TOL, (dx, do)
    for q in range(N):
        k = int(hdr["n_obs"][q])
        assert _kernel_of(api, 1, k, **desc) == "generic"
        rq = rows[int(off[q]):int(off[q + 1])] if k else None
        one = sol.solve_host(hdr[q:q + 1], rq, np.array([0, k * P], dtype=np.uint64) if k else None, sfc[q:q + 1])
        assert one["status"][0] == G["status"][q], (q, k)
        assert np.array_equal(one["x"][0], G["x"][q]) and one["obj"][0] == G["obj"][q], (q, k, np.abs(one["x"][0] - G["x"][q]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("M,dim,lsc_mode,forced", [(12, 3, False, False), (5, 3, True, True)], ids=["M12_dlsc", "M5_lsc_forced"])
def test_an_instance_beyond_n_obs_max_is_refused_and_the_others_are_untouched(api, oracle, torch_cuda, monkeypatch, M, dim, lsc_mode, forced):
    """The device entry with n_obs_max = 8 and ONE header that claims 9 neighbours: that instance is refused -- STATUS_CAPACITY, x_out = p0
    on every axis (there is no x_init), never truncated -- and every other instance is bit for bit what it is without the claim."""
    from lsc_dr_planner_amd import synth

    torch = torch_cuda
    _force(monkeypatch, forced)
    N, n_obs, bad = 12, 8, 5
    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=7)
    desc = dict(M=M, dim=dim, planner_mode=_mode(api, lsc_mode), world_min=sw.world_min, world_max=sw.world_max)
    assert _kernel_of(api, N, n_obs, **desc) == "generic"
    sol = api.Solver(api.make_desc(**desc))
    hdr, rows, off, sfc = api.batch_from_swarm(sw.build(), n_obs, M)
    rows = np.concatenate([rows, np.zeros(6 * M, api.ROW_DTYPE)])  # (room for a ninth neighbour behind every instance: nothing may read it)
    A = _solve_device(api, torch, sol, hdr, rows, off, sfc, n_obs)
    assert (A["status"] == 0).all(), A["status"]
    hdr2 = hdr.copy()
    hdr2["n_obs"][bad] = n_obs + 1
    B = _solve_device(api, torch, sol, hdr2, rows, off, sfc, n_obs)
    assert B["status"][bad] == api.STATUS_CAPACITY
    assert np.array_equal(B["x"][bad].reshape(dim, 6 * M), np.repeat(hdr["p0"][bad][:dim, None], 6 * M, axis=1))
    keep = np.arange(N) != bad
    assert np.array_equal(B["status"][keep], A["status"][keep])
    assert np.array_equal(B["x"][keep], A["x"][keep]) and np.array_equal(B["obj"][keep], A["obj"][keep])


# ---- the LDS boundary ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("lsc_mode", [True, False], ids=["lsc", "dlsc"])
def test_as_many_neighbours_as_the_lds_of_a_cu_holds(api, oracle, torch_cuda, lsc_mode):
    """M = 12 in 3-D with n_obs = max_obstacles() (60 with the end stop, 55 without): the launch whose LDS carve fills the CU's 160 KB -- OPTIMAL at the oracle's optimum on
    two replans.  One neighbour more is refused by the host-pointer entry with ERR_UNSUPPORTED before anything is launched (the check
    sits in front of every launch of the call: csrc/lscqp_api.hip, lscqp_solve_batch_device_internal_)."""
    from lsc_dr_planner_amd import synth

    M, dim = 12, 3
    desc = dict(M=M, dim=dim, planner_mode=_mode(api, lsc_mode))
    sol = api.Solver(api.make_desc(**desc))
    cap = sol.max_obstacles()
    assert cap == (60 if lsc_mode else 55)
    assert _kernel_of(api, cap + 8, cap, **desc) == "generic"
    _swarm_vs_oracle(api, oracle, M, dim, cap, lsc_mode, N=cap + 8, steps=2, seed=13)
    N = cap + 8
    sw = synth.Swarm(N, M=M, dim=dim, n_obs=cap + 1, seed=13)
    assert sw.n_obs == cap + 1
    hdr, rows, off, sfc = api.batch_from_swarm(sw.build(), sw.n_obs, M)
    hdr["n_obs"][:-1] = cap  # (one instance with cap + 1 is enough: the launch is sized by the largest)
    sol = api.Solver(api.make_desc(world_min=sw.world_min, world_max=sw.world_max, **desc))
    with pytest.raises(api.LscqpError) as e:
        sol.solve_host(hdr, rows, off, sfc)
    assert e.value.code == api.ERR_UNSUPPORTED and "holds %d obstacles" % (cap + 1) in str(e.value), e.value
    hdr["n_obs"][-1] = cap  # the same handle, the same buffers, one neighbour less: served
    assert (sol.solve_host(hdr, rows, off, sfc)["status"] == 0).all()


# ---- float32 rows --------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,dim,n_obs,seed,forced", [(64, 5, 3, 20, 1, True), (24, 12, 3, 20, 8, False)], ids=["M5_forced", "M12"])
def test_f32_rows_on_the_run_time_shaped_kernel(api, torch_cuda, monkeypatch, N, M, dim, n_obs, seed, forced):
    """tests/test_row_format.py's assertion on this kernel's `rows_f32` branch: the arithmetic stays fp64, so the result on float32 rows
    equals, bit for bit, the result on fp64 rows that hold the same float values."""
    from lsc_dr_planner_amd import synth

    _force(monkeypatch, forced)
    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=seed)
    b = sw.build()
    hdr, rows, off, sfc = api.batch_from_swarm(b, sw.n_obs, M)
    desc = dict(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max)
    assert _kernel_of(api, N, n_obs, row_format=api.ROWS_F32, **desc) == "generic" and _kernel_of(api, N, n_obs, **desc) == "generic"
    s32 = api.Solver(api.make_desc(row_format=api.ROWS_F32, **desc))
    s64 = api.Solver(api.make_desc(**desc))
    r32 = s32.rows_in_format(rows)
    widened = np.zeros(r32.shape, api.ROW_DTYPE)
    for f in ("nx", "ny", "nz", "b"):
        widened[f] = r32[f]
    x0 = api.x_init_from_swarm(b, dim)
    A = s32.solve_host(hdr, r32, off, sfc, x_init=x0)
    B = s64.solve_host(hdr, widened, off, sfc, x_init=x0)
    assert (A["status"] == 0).all()
    assert np.array_equal(A["x"], B["x"]) and np.array_equal(A["obj"], B["obj"]) and np.array_equal(A["status"], B["status"])
    assert np.array_equal(A["info"]["iterations"], B["info"]["iterations"])
    # against the fp64 rows of the generator the solution moves by the float32 rounding of b (|b| <~ 30 m: 2e-6 m), not more
    Cc = s64.solve_host(hdr, rows, off, sfc, x_init=x0)
    assert np.abs(A["x"] - Cc["x"]).max() <= 2e-5
