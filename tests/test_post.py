"""Post-solve epilogue: isSolValid + getStateAt + doStep on the device against the oracle."""
import numpy as np
import pytest

from tests import helpers as H


def test_validate_step_oracle_on_solved_swarm(oracle):
    """Solutions of the QP are valid by construction; pushing a control point out of its box or stretching the first
    segment beyond the velocity limit must flip the verdict (reference src/traj_planner.cpp:992-1042)."""
    from lsc_dr_planner_amd import synth

    N, M, dim = 12, 5, 3
    sw = synth.Swarm(N, M=M, dim=dim, n_obs=6, seed=11)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True, world_min=sw.world_min, world_max=sw.world_max)
    b = sw.build()
    ag, lsc, off, sfc = H.swarm_oracle_inputs(oracle, sw, b)
    R = oracle.solve_batch(cls, ag, lsc, off, sfc, threads=4)
    assert (R["status"] == 0).all()
    for q in range(N):
        ok, st = oracle.validate_step(cls, ag[q], b["sfc"][q], R["x"][q], 0.1)
        assert ok == 1
        pos, vel, acc = oracle.state_at(cls, np.float32(R["x"][q]).astype(np.float64), 0.1)
        assert np.allclose(st[:3], np.float32(pos)) and np.allclose(st[3:6], np.float32(vel)) and np.allclose(st[6:], np.float32(acc))
        x2 = R["x"][q].copy()
        x2[0 * M * 6 + 6 * 2 + 4] = b["sfc"]["bmax"][q, 2, 0] + 1e-3  # control point (m=2, i=4) beyond its box in x
        assert oracle.validate_step(cls, ag[q], b["sfc"][q], x2, 0.1)[0] == 0
        x3 = R["x"][q].copy()
        x3[0 * M * 6 + 3:0 * M * 6 + 6] += 2.0  # 2 m within one segment: |v| far above 1.01 * vmax
        assert oracle.validate_step(cls, ag[q], None if False else b["sfc"][q], x3, 0.1)[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,dim,n_obs,seed", [(32, 5, 3, 12, 3), (10, 10, 2, 9, 2)])
def test_gpu_validate_step_matches_oracle(api, oracle, N, M, dim, n_obs, seed):
    import torch

    from lsc_dr_planner_amd import synth

    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=seed)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True, world_min=sw.world_min, world_max=sw.world_max)
    sol = api.Solver(api.make_desc(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max))
    b = sw.build()
    hdr, rows, off, sfc = api.batch_from_swarm(b, sw.n_obs, M)
    r = sol.solve_host(hdr, rows, off, sfc)
    assert (r["status"] == 0).all()
    x = r["x"].copy()
    # make a third of the batch invalid in the two ways isSolValid knows
    for q in range(0, N, 3):
        if q % 2 == 0:
            x[q, 0 * M * 6 + 6 * (M - 1) + 2] = b["sfc"]["bmin"][q, M - 1, 0] - 1e-3
        else:
            x[q, 1 * M * 6 + 3:1 * M * 6 + 6] += 2.0
    z2d = float(b["p0"][0][2])
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_x = torch.from_numpy(x).to(dev)
    d_valid = torch.full((N,), -1, dtype=torch.int32, device=dev)
    d_state = torch.zeros(N * 9, dtype=torch.float64, device=dev)
    for ts in (0.1, 0.2):  # multisim_time_step < dt and == dt (reference src/param.cpp:134-148)
        sol.validate_step_device(N, ts, d_x, up(hdr), up(sfc), d_valid, d_state, z_2d=z2d)
        torch.cuda.synchronize()
        got_v, got_s = d_valid.cpu().numpy(), d_state.cpu().numpy().reshape(N, 9)
        ag, _, _, _ = H.swarm_oracle_inputs(oracle, sw, b)
        for q in range(N):
            ok, st = oracle.validate_step(cls, ag[q], b["sfc"][q], x[q], ts, z2d)
            assert got_v[q] == ok, (q, ts)
            # same float32 control points, fp64 Bernstein evaluation on both sides, float32 result: at most one ulp
            assert np.allclose(got_s[q], st, rtol=2e-7, atol=1e-7), (q, got_s[q], st)
        assert got_v.sum() < N and got_v.sum() >= N - (N + 2) // 3


# ---- safety metrics (reference src/multi_sync_simulator.cpp:486-577) -----------------------------------------------
def _const_plans(pos, M, dim):
    """Plans whose control points all equal `pos` (n, 3): getStateAt(0) returns exactly that position."""
    n = pos.shape[0]
    x = np.zeros((n, dim, M, 6))
    for k in range(dim):
        x[:, k] = pos[:, k, None, None]
    return x.reshape(n, -1)


def test_safety_ratio_oracle_reproduces_reference_summary(oracle):
    """The reference's own run: positions of its 10 agents at every logged time (log/simulation_*_LSC_10agents.csv) must
    give the safety_ratio_agent of its summary CSV (1.02089) and zero velocity / acceleration excess."""
    g = H.load_golden("sim_log_states")
    M, dim = 10, 2
    cls = oracle.make_class(M=M, dim=dim, use_sfc=False, world_min=[-5, -5, 0], world_max=[5, 5, 2.5])
    ag = np.zeros(10, oracle.AGENT_DTYPE)
    ag["vmax"], ag["amax"] = g["vmax"], g["amax"]
    best = np.inf
    for p in g["pos"]:
        p = np.array(p)
        out = oracle.safety_metrics(cls, ag, _const_plans(p, M, dim), g["radius"], g["downwash"], 1, 0.1, z_2d=p[0, 2])
        best = min(best, out[:, 0].min())
    # the log prints 6 significant digits -> positions to 5e-6 m -> ratio to ~3e-5
    assert abs(best - g["summary"]["safety_ratio_agent"]) <= 5e-5, best
    v, a = np.array(g["vel"]), np.array(g["acc"])
    assert max(0.0, ((v - g["vmax"]) / g["vmax"]).max()) == g["summary"]["vel_excess_ratio"] == 0.0
    assert max(0.0, ((a - g["amax"]) / g["amax"]).max()) == g["summary"]["acc_excess_ratio"] == 0.0


def test_safety_metrics_oracle_against_numpy(oracle):
    from lsc_dr_planner_amd import synth

    N, M, dim = 14, 5, 3
    sw = synth.Swarm(N, M=M, dim=dim, n_obs=6, seed=5)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True, world_min=sw.world_min, world_max=sw.world_max)
    b = sw.build()
    ag, lsc, off, sfc = H.swarm_oracle_inputs(oracle, sw, b)
    R = oracle.solve_batch(cls, ag, lsc, off, sfc, threads=4)
    ag["vmax"][:, 0] = 0.002  # for the metrics only: a limit the plans exceed in +x (the reference's ratio is signed)
    rad = np.full(N, sw.radius)
    dwv = np.full(N, sw.downwash)
    rad[2], dwv[2] = 0.25, 1.2
    out = oracle.safety_metrics(cls, ag, R["x"], rad, dwv, 3, 0.05)
    xf = np.float32(R["x"]).astype(np.float64)
    for a in range(N):
        best, bkey, vex = np.inf, None, 0.0
        for s in range(3):
            pa, va, _ = oracle.state_at(cls, xf[a], s * 0.05)
            vex = max(vex, (np.float32(va[0]) - 0.002) / 0.002)
            for j in range(N):
                if j == a:
                    continue
                pj, _, _ = oracle.state_at(cls, xf[j], s * 0.05)
                dwn = (dwv[a] * rad[a] + dwv[j] * rad[j]) / (rad[a] + rad[j])
                d = np.float32(pa) - np.float32(pj)
                d[2] = np.float32(d[2] / dwn)
                r = np.sqrt(float(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))) / (rad[a] + rad[j])
                if r < best:
                    best, bkey = r, (j, s)
        assert abs(out[a, 0] - best) <= 1e-7 * best and (out[a, 1], out[a, 2]) == bkey
        assert abs(out[a, 3] - max(vex, 0.0)) <= 1e-6
    assert out[:, 3].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,dim,n_obs,first,n_loc,seed", [(64, 5, 3, 12, 0, 64, 3), (300, 5, 3, 8, 100, 77, 4), (10, 10, 2, 9, 0, 10, 2)])
def test_gpu_safety_metrics_match_oracle(api, oracle, N, M, dim, n_obs, first, n_loc, seed):
    import torch

    from lsc_dr_planner_amd import synth

    sw = synth.Swarm(N, M=M, dim=dim, n_obs=n_obs, seed=seed)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True, world_min=sw.world_min, world_max=sw.world_max)
    sol = api.Solver(api.make_desc(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max))
    b = sw.build()
    hdr, rows, off, sfc = api.batch_from_swarm(b, sw.n_obs, M)
    r = sol.solve_host(hdr, rows, off, sfc)
    x = r["x"]
    hdr["vmax"][:, 0] = 0.002  # for the metrics only: a limit the plans exceed in +x (the reference's ratio is signed)
    rad = np.full(N, sw.radius)
    dwv = np.full(N, sw.downwash)
    rad[1], dwv[1] = 0.25, 1.2
    z2d = float(b["p0"][0][2])
    ag = np.zeros(n_loc, oracle.AGENT_DTYPE)
    ag["vmax"], ag["amax"] = hdr["vmax"][first:first + n_loc], hdr["amax"][first:first + n_loc]
    want = oracle.safety_metrics(cls, ag, x, rad, dwv, 2, 0.05, first=first, z_2d=z2d)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_out = torch.zeros(n_loc * api.SAFETY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    sol.safety_metrics_device(n_loc, first, N, 2, 0.05, torch.from_numpy(x.copy()).to(dev), torch.from_numpy(rad).to(dev),
                              torch.from_numpy(dwv).to(dev), up(hdr[first:first + n_loc]), d_out, z_2d=z2d)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(api.SAFETY_DTYPE)
    # same float32 states and float32 distance arithmetic on both sides: the Bernstein evaluation may differ in the last
    # fp64 bit before the float32 rounding of a position (one float32 ulp of a 10 m coordinate = 1e-6 m)
    assert np.abs(got["safety_ratio"] - want[:, 0]).max() <= 1e-5
    same = got["closest_agent"] == want[:, 1].astype(np.int32)
    assert same.mean() >= 0.98 and (got["sample"][same] == want[same, 2].astype(np.int32)).all()  # exact ties may swap
    assert np.abs(got["vel_excess_ratio"] - want[:, 3:6]).max() <= 1e-5 and np.abs(got["acc_excess_ratio"] - want[:, 6:9]).max() <= 1e-5
    assert got["vel_excess_ratio"][:, 0].max() > 0  # the tightened limit is really exceeded somewhere


def _obstacle_table(api, N, dim, world_min, world_max, rng):
    """A handful of non-agent obstacles as the constraint generator takes them (lscqp_obstacle), one of them "real" (skipped by the metric)."""
    obs = np.zeros(7, api.OBSTACLE_DTYPE)
    lo, hi = np.array(world_min, dtype=np.float64), np.array(world_max, dtype=np.float64)
    obs["position"] = lo + rng.uniform(0.1, 0.9, (7, 3)) * (hi - lo)
    obs["velocity"] = rng.uniform(-0.5, 0.5, (7, 3))
    obs["radius"] = rng.uniform(0.1, 0.6, 7)
    obs["downwash"] = rng.uniform(1.0, 3.0, 7)
    obs["max_acc"] = 1.0
    obs["type"] = 0
    obs["type"][3] = api.OBSTACLE_REAL  # :531-532
    obs["position"][3] = obs["position"][0]  # would win every minimum if it were not skipped ...
    obs["radius"][3] = 1e-3                  # (tiny radius sum -> huge ratio? no: make it the NEAREST in ratio terms below)
    return obs


def test_safety_obstacles_oracle_against_numpy(oracle, api):
    """safety_ratio_obs (reference src/multi_sync_simulator.cpp:527-557) restated in numpy, expression by expression: the mixed
    downwash (:538-540), ellipsoidalDistance in point3d = float32 arithmetic (include/util.hpp:155-159), the ratio in double, the first
    strict minimum in (sample, obstacle) order, "real" obstacles skipped, +inf / -1 when there is nothing to compare with."""
    from lsc_dr_planner_amd import synth

    N, M, dim = 9, 5, 3
    sw = synth.Swarm(N, M=M, dim=dim, n_obs=4, seed=11)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True, world_min=sw.world_min, world_max=sw.world_max)
    b = sw.build()
    ag, lsc, off, sfc = H.swarm_oracle_inputs(oracle, sw, b)
    R = oracle.solve_batch(cls, ag, lsc, off, sfc, threads=4)
    rng = np.random.default_rng(5)
    obs = _obstacle_table(api, N, dim, sw.world_min, sw.world_max, rng)
    tab = np.c_[obs["position"], obs["radius"], obs["downwash"]]
    skip = (obs["type"] == api.OBSTACLE_REAL).astype(np.int32)
    rad, dwv = np.full(N, sw.radius), np.full(N, sw.downwash)
    rad[2], dwv[2] = 0.25, 1.2
    out = oracle.safety_obstacles(cls, N, R["x"], rad, dwv, tab, 3, 0.05, skip=skip)
    xf = np.float32(R["x"]).astype(np.float64)
    for a in range(N):
        best, key = np.inf, (-1, -1)
        for s in range(3):
            pa, _, _ = oracle.state_at(cls, xf[a], s * 0.05)
            for o in range(len(obs)):
                if skip[o]:
                    continue
                dwn = (obs["radius"][o] * obs["downwash"][o] + rad[a] * dwv[a]) / (rad[a] + obs["radius"][o])
                d = np.float32(pa) - np.float32(obs["position"][o])
                d[2] = np.float32(np.float64(d[2]) / dwn)
                r = np.sqrt(float(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))) / (rad[a] + obs["radius"][o])
                if r < best:
                    best, key = r, (o, s)
        assert out[a, 0] == best and (out[a, 1], out[a, 2]) == key, (a, out[a], best, key)
    assert not (out[:, 1] == 3).any()
    # no obstacle that counts: SP_INFINITY, no index
    none = oracle.safety_obstacles(cls, N, R["x"], rad, dwv, tab[3:4], 3, 0.05, skip=np.ones(1, np.int32))
    assert np.isinf(none[:, 0]).all() and (none[:, 1] == -1).all() and (none[:, 2] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,dim,first,n_loc,seed", [(64, 5, 3, 0, 64, 3), (300, 5, 3, 100, 77, 4), (10, 10, 2, 0, 10, 2)])
def test_gpu_safety_obstacles_match_oracle(api, oracle, N, M, dim, first, n_loc, seed):
    """lscqp_safety_obstacles_device against the oracle's restatement of src/multi_sync_simulator.cpp:527-557 on solved plans, with the
    obstacle table lscqp_generate_lsc_obstacles_device takes (a "real" entry included, which both sides skip)."""
    import torch

    from lsc_dr_planner_amd import synth

    sw = synth.Swarm(N, M=M, dim=dim, n_obs=8, seed=seed)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True, world_min=sw.world_min, world_max=sw.world_max)
    sol = api.Solver(api.make_desc(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max))
    b = sw.build()
    hdr, rows, off, sfc = api.batch_from_swarm(b, sw.n_obs, M)
    x = sol.solve_host(hdr, rows, off, sfc)["x"]
    rng = np.random.default_rng(seed)
    obs = _obstacle_table(api, N, dim, sw.world_min, sw.world_max, rng)
    z2d = float(b["p0"][0][2])
    if dim == 2:
        obs["position"][:, 2] = z2d + rng.uniform(-0.3, 0.3, len(obs))
    rad, dwv = np.full(N, sw.radius), np.full(N, sw.downwash)
    rad[1], dwv[1] = 0.25, 1.2
    skip = (obs["type"] == api.OBSTACLE_REAL).astype(np.int32)
    want = oracle.safety_obstacles(cls, n_loc, x, rad, dwv, np.c_[obs["position"], obs["radius"], obs["downwash"]], 2, 0.05, first=first, z_2d=z2d, skip=skip)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_out = torch.zeros(n_loc * api.SAFETY_OBS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    sol.safety_obstacles_device(n_loc, first, N, 2, 0.05, torch.from_numpy(x.copy()).to(dev), torch.from_numpy(rad).to(dev), torch.from_numpy(dwv).to(dev),
                                len(obs), up(obs), d_out, z_2d=z2d)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(api.SAFETY_OBS_DTYPE)
    # (the Bernstein evaluation of a position may differ in the last fp64 bit before its float32 rounding: one float32 ulp of a 10 m coordinate)
    assert np.abs(got["safety_ratio_obs"] - want[:, 0]).max() <= 1e-5 and not (got["closest_obstacle"] == 3).any()
    same = got["closest_obstacle"] == want[:, 1].astype(np.int32)
    assert same.mean() >= 0.98 and (got["sample"][same] == want[same, 2].astype(np.int32)).all()
    exact = got["safety_ratio_obs"] == want[:, 0]
    assert exact.mean() >= 0.9  # IEEE division and square root on both sides: bit-for-bit wherever the float32 positions agree
    # nothing to compare with: SP_INFINITY and no index, like the reference's untouched running minimum
    sol.safety_obstacles_device(n_loc, first, N, 2, 0.05, torch.from_numpy(x.copy()).to(dev), torch.from_numpy(rad).to(dev), torch.from_numpy(dwv).to(dev),
                                0, None, d_out, z_2d=z2d)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(api.SAFETY_OBS_DTYPE)
    assert np.isinf(got["safety_ratio_obs"]).all() and (got["closest_obstacle"] == -1).all() and (got["sample"] == -1).all()


# ---- constructed cases (tests/post_cases.py): no QP solve, every expected result stated by construction ----------------------------
import functools  # noqa: E402

from tests import post_cases as PC  # noqa: E402

_VALIDATE_CLASSES = [(5, 3), (12, 3), (5, 2), (12, 2)]
# The device's safety ratio against the fp64 restatement (IEEE division and square root).  The kernel's reciprocal / reciprocal square root
# with Newton steps promise "the last bit or two"; the bar is the loosest one the cases allow -- a float32 slip anywhere in the ratio is
# 6e-8 -- until the largest deviation has been measured on an MI355X (every test prints its own; NOTES.md section 25), and is then to
# stand at four times that figure, never looser than this.
RATIO_RTOL = 1e-13


def _orc_boxes(oracle, bmin, bmax):
    box = np.zeros(len(bmin), oracle.BOX_DTYPE)
    box["bmin"], box["bmax"] = bmin, bmax
    return box


def _orc_agent(oracle, vmax, amax):
    ag = np.zeros(1, oracle.AGENT_DTYPE)
    ag["vmax"], ag["amax"] = vmax, amax
    return ag[0]


@functools.lru_cache(maxsize=None)
def _validate_groups(M, dim):
    return PC.validate_groups(M, dim)


@pytest.mark.parametrize("M,dim", _VALIDATE_CLASSES)
def test_validate_constructed_cases_on_oracle(oracle, M, dim):
    """Every constructed isSolValid / doStep case gives its by-construction verdict on the oracle and on the numpy restatement; without
    corridors the out-of-box plans are valid."""
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True)
    cls_off = oracle.make_class(M=M, dim=dim, use_sfc=False)
    n_cases = 0
    for g in _validate_groups(M, dim):
        v_np, s_np = PC.validate_step_np(g["x4"], g["vmax"], g["amax"], g["bmin"], g["bmax"], PC.DT, g["time_step"], g["z_2d"])
        v_off, _ = PC.validate_step_np(g["x4"], g["vmax"], g["amax"], None, None, PC.DT, g["time_step"], g["z_2d"])
        for q in range(g["n"]):
            tag = (g["name"], g["names"][q])
            ag = _orc_agent(oracle, g["vmax"][q], g["amax"][q])
            ok, st = oracle.validate_step(cls, ag, _orc_boxes(oracle, g["bmin"][q], g["bmax"][q]), g["x4"][q].reshape(-1), g["time_step"], g["z_2d"])
            assert ok == g["valid"][q] == v_np[q], (tag, ok, v_np[q])
            assert np.allclose(st, s_np[q], rtol=2e-7, atol=1e-7), (tag, st, s_np[q])
            ok_off, _ = oracle.validate_step(cls_off, ag, None, g["x4"][q].reshape(-1), g["time_step"], g["z_2d"])
            box_case = g["name"].startswith(("box", "skipped", "z2d"))
            assert ok_off == v_off[q] == (1 if box_case else g["valid"][q]), tag
            n_cases += 1
        if "piecewise_point" in g:  # a piecewise-constant plan: the state is the segment's point, exactly, and at rest
            want = np.r_[g["piecewise_point"][:dim], [g["z_2d"]] * (3 - dim), np.zeros(6)]
            assert np.array_equal(s_np[0], want), (g["name"], s_np[0], want)
    assert n_cases >= 60


@pytest.mark.parametrize("M,dim", [(5, 3), (12, 2)])
def test_commit_case_on_oracle(oracle, api, M, dim):
    c = PC.commit_case(M, dim, api)
    cls = oracle.make_class(M=M, dim=dim, use_sfc=True)
    assert not np.isnan(c["chosen"]).any() and np.isnan(c["x_new"]).any() and np.isnan(c["x_init"]).any()
    box = _orc_boxes(oracle, np.full((M, 3), -1.0), np.full((M, 3), 1.0))
    v_np, _ = PC.validate_step_np(c["chosen"], np.tile(PC.VMAX, (c["n"], 1)), np.tile(PC.AMAX, (c["n"], 1)), np.full((c["n"], M, 3), -1.0),
                                  np.full((c["n"], M, 3), 1.0), PC.DT, 0.5 * PC.DT, PC.BASE[2])
    for q in range(c["n"]):
        ok, _ = oracle.validate_step(cls, _orc_agent(oracle, PC.VMAX, PC.AMAX), box, c["chosen"][q].reshape(-1), 0.5 * PC.DT, PC.BASE[2])
        assert ok == c["valid"][q] == v_np[q], q


def _saf_arrays(n):
    return np.full(n, PC.SAF_RADIUS), np.ones(n), np.tile(PC.VMAX, (n, 1)), np.tile(PC.AMAX, (n, 1))


def _saf_np(x4, first=0, n_loc=None, vmax=None, amax=None, lo=0, hi=None):
    n = len(x4)
    n_loc = n - first if n_loc is None else n_loc
    rad, dwv, vm, am = _saf_arrays(n)
    vm, am = (vm if vmax is None else vmax)[first:first + n_loc], (am if amax is None else amax)[first:first + n_loc]
    return PC.safety_metrics_np(x4, rad, dwv, vm, am, first, n_loc, PC.SAF_SAMPLES, PC.SAF_STEP, PC.DT, 1.0, lo=lo, hi=hi)


def _saf_oracle(oracle, x4, first=0, n_loc=None, vmax=None, amax=None):
    n = len(x4)
    n_loc = n - first if n_loc is None else n_loc
    rad, dwv, vm, am = _saf_arrays(n)
    ag = np.zeros(n_loc, oracle.AGENT_DTYPE)
    ag["vmax"], ag["amax"] = (vm if vmax is None else vmax)[first:first + n_loc], (am if amax is None else amax)[first:first + n_loc]
    cls = oracle.make_class(M=PC.SAF_M, dim=3, use_sfc=False)
    return oracle.safety_metrics(cls, ag, PC.flat(x4), rad, dwv, PC.SAF_SAMPLES, PC.SAF_STEP, first=first)


_LATTICE_SIZES = [1, 2, 33, 255, 256, 257, 513]


@functools.lru_cache(maxsize=None)
def _lattice_case(n, kind):
    """(x4, by-construction [n][3], restatement [n][9]); kind: "plain", "perm" (ids shuffled), "late" (closest in segment 3 only)."""
    perm = np.random.default_rng(n).permutation(n) if kind == "perm" else None
    x4, want = PC.lattice(n, perm=perm, late=kind == "late")
    res = _saf_np(x4)
    assert np.array_equal(res[:, :3], want), (n, kind)  # the restatement gives the by-construction result, bit for bit
    assert not res[:, 3:].any()
    return x4, want, res


# (the oracle's loop is n^2 * samples evaluations of a trajectory: the shuffled and the late lattice are held to it at two sizes, and to
# the restatement -- which _lattice_case holds to the by-construction result -- at all of them)
@pytest.mark.parametrize("n,kind", [(n, "plain") for n in _LATTICE_SIZES] + [(n, k) for k in ("perm", "late") for n in (2, 257)])
def test_safety_lattice_on_oracle(oracle, n, kind):
    """Exact ties everywhere: the first strict minimum in (sample, j) order is the lower id at sample 0 (the first sample inside
    segment 3 for the late plans); a lone agent gets +inf, -1, -1."""
    x4, want, _ = _lattice_case(n, kind)
    got = _saf_oracle(oracle, x4)
    assert np.array_equal(got[:, :3], want) and not got[:, 3:].any()
    if n > 1:
        assert (want[:, 2] == (6 if kind == "late" else 0)).all()
        if kind != "perm":  # agent 0 sees 1, interior agents the LOWER neighbour, the last two each other
            assert np.array_equal(want[:, 1], np.r_[1, np.arange(n - 3), n - 1, n - 2] if n > 2 else [1, 0])


def test_safety_lattice_restatement_all_sizes():
    for n in _LATTICE_SIZES:
        for kind in ("plain", "perm", "late"):
            _lattice_case(n, kind)


@functools.lru_cache(maxsize=None)
def _scattered_case():
    x4 = PC.scattered(300, 21)
    return x4, _saf_np(x4)


@functools.lru_cache(maxsize=None)
def _excess_case():
    x4, vmax, amax, want_v, want_a = PC.excess_case()
    res = _saf_np(x4, vmax=vmax, amax=amax)
    # 0.5 to one float32 ulp (relative) where the limit is exceeded by half, exactly 0 at -2 vmax (the ratio is signed) and at 0.99 vmax
    for got, want in ((res[:, 3:6], want_v), (res[:, 6:9], want_a)):
        assert (got[want == 0] == 0).all() and (np.abs(got[want > 0] - 0.5) <= 0.5 * 2.0 ** -23).all(), got
        assert (want > 0).sum() == 3
    return x4, vmax, amax, res


def test_safety_scattered_and_excess_on_oracle(oracle):
    x4, res = _scattered_case()
    got = _saf_oracle(oracle, x4)
    assert np.array_equal(got, res)  # IEEE division and square root on both sides
    x4, vmax, amax, res = _excess_case()
    got = _saf_oracle(oracle, x4, vmax=vmax, amax=amax)
    assert np.array_equal(got[:, :3], res[:, :3]) and np.abs(got[:, 3:] - res[:, 3:]).max() <= 1e-15
    # the quadratic factor worked out in the builder, on the oracle: c_i = i^2 a / 2 is the constant acceleration 20 a / dt^2
    cls = oracle.make_class(M=PC.SAF_M, dim=3, use_sfc=False)
    x = np.zeros((1, 3, PC.SAF_M, 6))
    PC.set_quadratic(x, 0, 1, 2, 0.5, 0.0078125)
    PC.set_linear(x, 0, 1, 0, 0.5, 0.015625)
    for t in (0.2, 0.25, 0.3999):
        _, v, a = oracle.state_at(cls, x.reshape(-1), t)
        assert abs(a[2] - PC.quadratic_acceleration(0.0078125)) <= 1e-12 and abs(v[0] - PC.linear_velocity(0.015625)) <= 1e-13 and abs(a[0]) <= 1e-11
        assert abs(v[2] - PC.quadratic_velocity(0.0078125, (t - 0.2) / 0.2)) <= 1e-12


@functools.lru_cache(maxsize=None)
def _missions_case():
    """(x4, vmax, amax, restatement [n][9] mission by mission)."""
    x4, vmax, amax = PC.missions_case()
    off = PC.MISSION_OFFSETS
    res = np.concatenate([_saf_np(x4, first=lo, n_loc=hi - lo, vmax=vmax, amax=amax, lo=lo, hi=hi) for lo, hi in zip(off[:-1], off[1:])])
    return x4, vmax, amax, res


def test_safety_missions_case_on_oracle(oracle):
    """Every mission is the plain form on its slice alone with ids shifted to global; the mission of one gets +inf, -1, -1; the two
    agents 0.1 m apart across a mission boundary do not see each other (and would, in one swarm)."""
    x4, vmax, amax, res = _missions_case()
    off = PC.MISSION_OFFSETS
    for lo, hi in zip(off[:-1], off[1:]):
        got = _saf_oracle(oracle, x4[lo:hi], vmax=vmax[lo:hi], amax=amax[lo:hi])
        got[:, 1] = np.where(got[:, 1] >= 0, got[:, 1] + lo, -1)
        assert np.array_equal(got[:, :3], res[lo:hi, :3]) and np.abs(got[:, 3:] - res[lo:hi, 3:]).max() <= 1e-15, (lo, hi)
    assert np.isinf(res[0, 0]) and res[0, 1] == res[0, 2] == -1
    assert res[31, 1] != 32 and res[32, 1] != 31 and min(res[31, 0], res[32, 0]) > 0.1 / (2 * PC.SAF_RADIUS) * 1.01
    one = _saf_np(x4, vmax=vmax, amax=amax)
    assert one[31, 1] == 32 and one[32, 1] == 31
    assert (res[[0, 5, 40, 96, 353], 3:6].max(axis=1) > 0.1).all() and np.count_nonzero(res[:, 3:6]) == 5  # (limits grow with the id)


_OBS_SIZES = [1, 255, 256, 257]


@functools.lru_cache(maxsize=None)
def _obstacles_case(n):
    from lsc_dr_planner_amd import api

    x4, obs = PC.obstacles_case(n, api)
    rad, dwv = np.full(n, PC.SAF_RADIUS), np.ones(n)
    skip = (obs["type"] == api.OBSTACLE_REAL).astype(np.int32)
    res = PC.safety_obstacles_np(x4, rad, dwv, obs["position"], obs["radius"], obs["downwash"], skip, 0, n, 2, PC.SAF_STEP, PC.DT, 1.0)
    # by construction: never the "real" obstacle on the line, never the upper twin, never the far one; the twins win far from obstacle 0
    assert np.isin(res[:, 1], (0, 1)).all() and (res[:, 2] == 0).all() and res[0, 1] == 0
    if n > 200:
        assert (res[120:, 1] == 1).all()
    return x4, obs, skip, res


@pytest.mark.parametrize("n", _OBS_SIZES)
def test_safety_obstacles_case_on_oracle(oracle, n):
    x4, obs, skip, res = _obstacles_case(n)
    cls = oracle.make_class(M=PC.SAF_M, dim=3, use_sfc=False)
    got = oracle.safety_obstacles(cls, n, PC.flat(x4), PC.SAF_RADIUS, 1.0, np.c_[obs["position"], obs["radius"], obs["downwash"]], 2, PC.SAF_STEP,
                                  skip=skip)
    assert np.array_equal(got, res)


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _validate_device(api, sol, g, use_sfc=True):
    """One launch over a group; a guard word and a guard state sit behind the batch.  Returns (valid[n], state[n][9])."""
    import torch

    n, M = g["n"], g["x4"].shape[2]
    hdr = np.zeros(n, api.HEADER_DTYPE)
    hdr["vmax"], hdr["amax"] = g["vmax"], g["amax"]
    sfc = np.zeros((n, M), api.BOX_DTYPE)
    sfc["bmin"], sfc["bmax"] = g["bmin"], g["bmax"]
    dev = torch.device("cuda", 0)
    d_valid = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    d_state = torch.full(((n + 1) * 9,), -7.0, dtype=torch.float64, device=dev)
    sol.validate_step_device(n, g["time_step"], torch.from_numpy(PC.flat(g["x4"])).to(dev), _up(hdr), _up(sfc) if use_sfc else None, d_valid, d_state,
                             z_2d=g["z_2d"])
    torch.cuda.synchronize()
    v, s = d_valid.cpu().numpy(), d_state.cpu().numpy().reshape(n + 1, 9)
    assert v[n] == -7 and (s[n] == -7.0).all()
    return v[:n], s[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("M,dim", _VALIDATE_CLASSES)
def test_gpu_validate_constructed_cases(api, oracle, M, dim):
    """The box margin on both sides at float32 bounds (element indices >= 64 at M = 12), the unjudged points of segment 0, the 1 %
    tolerance per axis, world_z_2d against the box, step times in, between and behind the segments, and the same plans without
    corridors: verdicts exactly the stated ones, states at the existing bar."""
    sol = api.Solver(api.make_desc(M=M, dim=dim, use_sfc=True))
    sol_off = api.Solver(api.make_desc(M=M, dim=dim, use_sfc=False))
    for g in _validate_groups(M, dim):
        v_np, s_np = PC.validate_step_np(g["x4"], g["vmax"], g["amax"], g["bmin"], g["bmax"], PC.DT, g["time_step"], g["z_2d"])
        v, s = _validate_device(api, sol, g)
        assert np.array_equal(v, g["valid"]) and np.array_equal(v, v_np), (g["name"], [g["names"][q] for q in np.flatnonzero(v != g["valid"])])
        assert np.allclose(s, s_np, rtol=2e-7, atol=1e-7), (g["name"], np.abs(s - s_np).max())
        assert not np.isnan(s).any()
        if "piecewise_point" in g:
            assert np.array_equal(s[0], s_np[0]), (g["name"], s[0], s_np[0])  # exact on both sides
        v_off, s_off = _validate_device(api, sol_off, g, use_sfc=False)  # the corridor pointer is NULL
        box_case = g["name"].startswith(("box", "skipped", "z2d"))
        assert np.array_equal(v_off, np.ones_like(v) if box_case else g["valid"]), g["name"]
        assert np.array_equal(s_off, s), g["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("M,dim", [(5, 3), (12, 2)])
def test_gpu_commit_validate(api, M, dim):
    """The chain's commit form: x_plan is the new plan where the QP is OPTIMAL and the initial trajectory otherwise, bit for bit (the
    other source is NaN and must not show anywhere), goal = hdr.goal, and the verdict and state are validate_step_device's on that plan."""
    import torch

    c = PC.commit_case(M, dim, api)
    n, nv = c["n"], dim * M * 6
    sol = api.Solver(api.make_desc(M=M, dim=dim, use_sfc=True))
    hdr = np.zeros(n, api.HEADER_DTYPE)
    hdr["vmax"], hdr["amax"], hdr["goal"] = PC.VMAX, PC.AMAX, c["goal"]
    sfc = np.zeros((n, M), api.BOX_DTYPE)
    sfc["bmin"], sfc["bmax"] = -1.0, 1.0
    dev = torch.device("cuda", 0)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(dev)  # noqa: E731
    d_plan = torch.full(((n + 1) * nv,), -7.0, dtype=torch.float64, device=dev)
    d_goal = torch.full(((n + 1) * 3,), -7.0, dtype=torch.float64, device=dev)
    d_valid = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    d_state = torch.full(((n + 1) * 9,), -7.0, dtype=torch.float64, device=dev)
    z0, ts = float(PC.BASE[2]), 0.5 * PC.DT
    sol.commit_validate_device(n, ts, torch.from_numpy(c["status"]).to(dev), t64(c["x_new"]), t64(c["x_init"]), d_plan, d_goal, _up(hdr), _up(sfc),
                               d_valid, d_state, z_2d=z0)
    torch.cuda.synchronize()
    plan, goal = d_plan.cpu().numpy().reshape(n + 1, nv), d_goal.cpu().numpy().reshape(n + 1, 3)
    valid, state = d_valid.cpu().numpy(), d_state.cpu().numpy().reshape(n + 1, 9)
    assert plan[:n].tobytes() == PC.flat(c["chosen"]).tobytes() and goal[:n].tobytes() == c["goal"].tobytes()
    assert (plan[n] == -7.0).all() and (goal[n] == -7.0).all() and valid[n] == -7 and (state[n] == -7.0).all()
    assert not np.isnan(plan).any() and not np.isnan(state).any() and not np.isnan(goal).any()
    g = dict(n=n, x4=c["chosen"], vmax=np.tile(PC.VMAX, (n, 1)), amax=np.tile(PC.AMAX, (n, 1)), bmin=np.full((n, M, 3), -1.0),
             bmax=np.full((n, M, 3), 1.0), time_step=ts, z_2d=z0)
    v, s = _validate_device(api, sol, g)
    assert np.array_equal(valid[:n], v) and np.array_equal(valid[:n], c["valid"]) and state[:n].tobytes() == s.tobytes()


def _safety_device(api, x4, first=0, n_loc=None, vmax=None, amax=None, offsets=None):
    """safety_metrics_device (offsets: the missions form) on plans x4 with every radius 0.15 and every downwash 1; a guard record behind
    the output."""
    import torch

    n = len(x4)
    n_loc = n - first if n_loc is None else n_loc
    rad, dwv, vm, am = _saf_arrays(n)
    hdr = np.zeros(n_loc, api.HEADER_DTYPE)
    hdr["vmax"], hdr["amax"] = (vm if vmax is None else vmax)[first:first + n_loc], (am if amax is None else amax)[first:first + n_loc]
    sol = api.Solver(api.make_desc(M=PC.SAF_M, dim=3, use_sfc=False))
    dev = torch.device("cuda", 0)
    size = api.SAFETY_DTYPE.itemsize
    d_out = torch.full(((n_loc + 1) * size,), 0xA5, dtype=torch.uint8, device=dev)
    args = (PC.SAF_SAMPLES, PC.SAF_STEP, torch.from_numpy(PC.flat(x4)).to(dev), torch.from_numpy(rad).to(dev), torch.from_numpy(dwv).to(dev), _up(hdr), d_out)
    if offsets is None:
        sol.safety_metrics_device(n_loc, first, n, *args)
    else:
        sol.safety_metrics_missions_device(offsets, *args)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[n_loc * size:] == 0xA5).all()
    return raw[:n_loc * size].view(api.SAFETY_DTYPE)


def _ratio_deviation(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(got), ~fin) and (got[~fin] > 0).all()
    return float((np.abs(got[fin] - want[fin]) / want[fin]).max()) if fin.any() else 0.0


def _check_safety(got, res, tag):
    """closest_agent and sample for 100 % of the agents, the ratio at RATIO_RTOL, the excess ratios at fp64 rounding."""
    assert np.array_equal(got["closest_agent"], res[:, 1].astype(np.int32)), (tag, np.flatnonzero(got["closest_agent"] != res[:, 1])[:8])
    assert np.array_equal(got["sample"], res[:, 2].astype(np.int32)), tag
    dev = _ratio_deviation(got["safety_ratio"], res[:, 0])
    print("safety ratio deviation %s: %.3e" % (tag, dev))
    assert dev <= RATIO_RTOL, (tag, dev)
    assert np.abs(got["vel_excess_ratio"] - res[:, 3:6]).max() <= 1e-15 and np.abs(got["acc_excess_ratio"] - res[:, 6:9]).max() <= 1e-15, tag
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "perm", "late"])
@pytest.mark.parametrize("n", _LATTICE_SIZES)
def test_gpu_safety_lattice(api, n, kind):
    """Tile tails (255, 256, 257, 513 trajectories), chunk tails, a lone agent and a closest agent alone in the last tile, with exact
    ties at every interior agent."""
    x4, want, res = _lattice_case(n, kind)
    got = _safety_device(api, x4)
    assert np.array_equal(got["closest_agent"], want[:, 1].astype(np.int32)) and np.array_equal(got["sample"], want[:, 2].astype(np.int32))
    _check_safety(got, res, ("lattice", n, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("first,n_loc", [(0, 257), (31, 33), (224, 33), (256, 1)])
def test_gpu_safety_blocks(api, first, n_loc):
    """Local blocks of a 257-agent swarm: chunk tails against every tile, the last agent alone."""
    for kind in ("plain", "perm"):
        x4, want, res = _lattice_case(257, kind)
        got = _safety_device(api, x4, first=first, n_loc=n_loc)
        _check_safety(got, res[first:first + n_loc], ("block", first, n_loc, kind))


@pytest.mark.gpu
def test_gpu_safety_ratio_accuracy_and_excess(api):
    """Scattered float32 positions (no exact square roots): the ratio against IEEE fp64 at RATIO_RTOL; the signed excess ratios: 0.5 where
    the limit is exceeded by half, exactly 0 at -2 vmax and at 0.99 vmax, per axis, for velocity and acceleration."""
    x4, res = _scattered_case()
    dev = _check_safety(_safety_device(api, x4), res, ("scattered", 300))
    assert dev < 1e-13
    x4, vmax, amax, res = _excess_case()
    got = _safety_device(api, x4, vmax=vmax, amax=amax)
    _check_safety(got, res, ("excess", len(x4)))
    for g, w in ((got["vel_excess_ratio"], res[:, 3:6]), (got["acc_excess_ratio"], res[:, 6:9])):
        assert (g[w == 0] == 0).all() and (np.abs(g[w > 0] - 0.5) <= 0.5 * 2.0 ** -23).all()


@pytest.mark.gpu
def test_gpu_safety_missions(api):
    """Missions of 1, 31, 32, 33 and 257 agents: each equals the plain form on its slice alone with ids shifted to global, bit for bit,
    and the restatement; the mission of one gets +inf, -1, -1; neighbours across a mission boundary do not see each other."""
    x4, vmax, amax, res = _missions_case()
    off = PC.MISSION_OFFSETS
    got = _safety_device(api, x4, vmax=vmax, amax=amax, offsets=off)
    _check_safety(got, res, ("missions", off[-1]))
    assert np.isinf(got["safety_ratio"][0]) and got["closest_agent"][0] == got["sample"][0] == -1
    assert got["closest_agent"][31] != 32 and got["closest_agent"][32] != 31
    for lo, hi in zip(off[:-1], off[1:]):
        alone = _safety_device(api, x4[lo:hi], vmax=vmax[lo:hi], amax=amax[lo:hi]).copy()
        alone["closest_agent"] = np.where(alone["closest_agent"] >= 0, alone["closest_agent"] + lo, -1)
        assert alone.tobytes() == got[lo:hi].tobytes(), (lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("n", _OBS_SIZES)
def test_gpu_safety_obstacles_ties_and_tails(api, n):
    """The 256-lane block tail and exact ties between obstacles: the lower index wins, the "real" obstacle on the agents' line is never
    chosen, and the ratio is the restatement's bit for bit (IEEE division and square root in the kernel)."""
    import torch

    x4, obs, skip, res = _obstacles_case(n)
    sol = api.Solver(api.make_desc(M=PC.SAF_M, dim=3, use_sfc=False))
    dev = torch.device("cuda", 0)
    size = api.SAFETY_OBS_DTYPE.itemsize
    d_out = torch.full(((n + 1) * size,), 0xA5, dtype=torch.uint8, device=dev)
    sol.safety_obstacles_device(n, 0, n, 2, PC.SAF_STEP, torch.from_numpy(PC.flat(x4)).to(dev), torch.from_numpy(np.full(n, PC.SAF_RADIUS)).to(dev),
                                torch.from_numpy(np.ones(n)).to(dev), len(obs), _up(obs), d_out)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[n * size:] == 0xA5).all()
    got = raw[:n * size].view(api.SAFETY_OBS_DTYPE)
    assert np.array_equal(got["closest_obstacle"], res[:, 1].astype(np.int32)) and np.array_equal(got["sample"], res[:, 2].astype(np.int32))
    assert got["safety_ratio_obs"].tobytes() == res[:, 0].tobytes()
