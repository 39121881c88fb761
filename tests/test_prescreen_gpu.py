"""The prescreen on the device (include/lscqp.h, csrc/lscqp_prescreen.hip), alone and in front of a solve.

Standalone entry, on the constructed cases (tests/prescreen_cases.py) and families A, B, C of tests/feasibility.py:
  R1 sound     every fired certificate passes the verifier (tests/prescreen_reference.py), and the exact referee never calls the instance FEASIBLE;
  R2 complete  max_cp t*_cp >= 1e-5  =>  fired;
  R3           max_cp t*_cp <= 0.9e-6  =>  not fired;
  the reported control point is the lowest with t*_cp >= 1e-5 whenever no lower one lies in the window; two calls give the same bytes; a
  captured graph replays them; an instance beyond the launch's obstacle capacity is not judged.
The three FIXED control points carry no verdict: the solver reads no LSC row there (src/traj_optimizer.cpp:404-406), so the cases that push
c0, c1 or c2 across a row must stay quiet -- R1 would fail otherwise.
Inside the solve, on every path that can carry a verdict: a fired instance is INFEASIBLE with ACTIVE_SET | PRESCREENED, 0 iterations, the
certificate's violation and the start as its point; every other instance equals the same call with the prescreen off bit for bit."""
import numpy as np
import pytest

from tests import feasibility as F
from tests import prescreen_cases as PC
from tests import prescreen_reference as PR

CHUNK = 64


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _certs(api, torch, sol, arrays, n_obs_max, stream=None):
    hdr, rows, off, sfc = arrays
    n = len(hdr)
    d = [_up(torch, hdr), _up(torch, sol.rows_in_format(rows)), _up(torch, np.ascontiguousarray(off, dtype=np.uint64)), _up(torch, sfc)]
    out = torch.full((n * api.PRESCREEN_CERT_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=d[0].device)
    sol.prescreen_device(n, n_obs_max, *d, out, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(api.PRESCREEN_CERT_DTYPE).copy(), d, out


def _model(O, ocls, inst, rows):
    ag, lsc, sfc = F.oracle_inputs(O, inst.hdr, rows, inst.sfc)
    return O.assemble(ocls, ag, lsc, sfc)


def _hold(api, O, ci, ocls, inst, rows, cert, t, fails, tag, referee_budget):
    """R1 - R3 and the reported control point for one instance; t: t*_cp [P] of the rows as the device read them."""
    label = PR.label_of(t.max())
    if cert["fired"]:
        try:
            PR.verify_cert(ci, inst.hdr, rows, _model(O, ocls, inst, rows), cert)
        except PR.CertError as e:
            fails.append("R1 %s: %s" % (tag, e))
        if referee_budget[0] > 0:
            referee_budget[0] -= 1
            ag, lsc, sfc = F.oracle_inputs(O, inst.hdr, rows, inst.sfc)
            v = F.judge_model(O.assemble(ocls, ag, lsc, sfc))
            if v.label == F.FEASIBLE:
                fails.append("R1 %s: fired, the referee says %r" % (tag, v))
        if label == PR.QUIET:
            fails.append("R3 %s: fired with max t* = %.3g" % (tag, t.max()))
        over = [cp for cp in range(3, ci.P) if t[cp] > PR.MUST_NOT_BAR]
        if over and t[over[0]] >= PR.MUST_FIRE_BAR and cert["control_point"] != over[0]:
            fails.append("control point %s: reported %d, lowest is %d" % (tag, cert["control_point"], over[0]))
    else:
        if label == PR.FIRE:
            fails.append("R2 %s: not fired with max t* = %.3g" % (tag, t.max()))
        if cert["control_point"] != -1 or cert["n_rows"] != 0 or cert["violation"] != 0.0:
            fails.append("%s: a quiet certificate is not blank" % tag)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f64", "f32"])
@pytest.mark.parametrize("shape", sorted(PC.SHAPES))
def test_prescreen_alone_on_the_constructed_cases(api, oracle, torch_cuda, shape, fmt):
    torch = torch_cuda
    cs = PC.build(api, shape)
    sol = api.Solver(cs.desc(api, row_format=api.ROWS_F32 if fmt == "f32" else api.ROWS_F64))
    ocls = cs.oracle_class(oracle)
    fails, fired, budget = [], 0, [10]
    for c0 in range(0, len(cs.cases), CHUNK):
        part = cs.cases[c0:c0 + CHUNK]
        arrays = PC.to_batch(api, part, cs.n_obs, cs.M)
        cert, d, _ = _certs(api, torch, sol, arrays, cs.n_obs)
        again, _, _ = _certs(api, torch, sol, arrays, cs.n_obs)
        assert cert.tobytes() == again.tobytes()
        for c, ct in zip(part, cert):
            rows = PC.rows_as_f32(c.inst.rows) if fmt == "f32" else c.inst.rows
            t = cs.base_t.copy()
            if c.kind != "fixed":
                for cp in c.cps:
                    t[cp] = PR.t_star_cp(cs.ci, c.inst.hdr, rows, c.inst.sfc, cp)
            fired += int(ct["fired"])
            _hold(api, oracle, cs.ci, ocls, c.inst, rows, ct, t, fails, "%s %s s=%s cp=%s" % (shape, c.kind, c.s, c.cps), budget)
        if c0 == 0:  # beyond the launch's capacity: not judged, whatever the rows say
            over, _, _ = _certs(api, torch, sol, arrays, cs.n_obs - 1)
            assert not over["fired"].any() and (over["control_point"] == -1).all()
    assert fired >= 30 and not fails, "\n".join(fails[:30])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(F.SHAPES))
def test_prescreen_alone_on_the_referees_families(api, oracle, torch_cuda, shape):
    torch = torch_cuda
    groups = F.build_groups(api, oracle, shape, judge_all=False)
    fails, fired, budget = [], 0, [40]
    for g in groups:
        ci = PR.ClassInfo(g.M, g.dim, g.world_min, g.world_max, comm_range=g.comm_range)
        sol = api.Solver(g.desc(api))
        ocls = g.oracle_class(oracle)
        for c0 in range(0, len(g.insts), CHUNK):
            part = g.insts[c0:c0 + CHUNK]
            cert, _, _ = _certs(api, torch, sol, F.to_batch(api, part, g.n_obs, g.M), g.n_obs)
            for i, ct in zip(part, cert):
                t = PR.t_star_all(ci, i.hdr, i.rows, i.sfc)
                fired += int(ct["fired"])
                _hold(api, oracle, ci, ocls, i, i.rows, ct, t, fails, "%s %s/%s %s" % (shape, g.name, i.family, i.params), budget)
    assert fired >= 10 and not fails, "\n".join(fails[:30])


@pytest.mark.gpu
def test_prescreen_captured_into_a_graph_replays(api, torch_cuda):
    torch = torch_cuda
    cs = PC.build(api, "m12")
    sol = api.Solver(cs.desc(api))
    part = cs.cases[:CHUNK]
    eager, d, _ = _certs(api, torch, sol, PC.to_batch(api, part, cs.n_obs, cs.M), cs.n_obs)
    assert eager["fired"].any() and not eager["fired"].all()
    out = torch.zeros(len(part) * api.PRESCREEN_CERT_DTYPE.itemsize, dtype=torch.uint8, device=d[0].device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            sol.prescreen_device(len(part), cs.n_obs, *d, out, stream=side)
    torch.cuda.synchronize()
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == eager.tobytes()


# ---- inside the solve ---------------------------------------------------------------------------------------------------------------

PATHS = ("device_small", "device_large", "host", "as_only", "as_off", "f32", "m9")


def _solve_device(api, torch, sol, arrays, n_obs, x_init=None):
    hdr, rows, off, sfc = arrays
    n = len(hdr)
    dev = torch.device("cuda", 0)
    x = torch.full((n * sol.nv,), 7.0, dtype=torch.float64, device=dev)
    obj = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    info = torch.zeros(n * api.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    xi = None if x_init is None else torch.from_numpy(np.ascontiguousarray(x_init)).to(dev)
    sol.solve_device(n, n_obs, _up(torch, hdr), _up(torch, sol.rows_in_format(rows)), _up(torch, np.ascontiguousarray(off, dtype=np.uint64)),
                     _up(torch, sfc), x, obj, st, info, d_x_init=xi)
    torch.cuda.synchronize()
    return dict(x=x.cpu().numpy().reshape(n, sol.nv), obj=obj.cpu().numpy(), status=st.cpu().numpy(), info=info.cpu().numpy().view(api.INFO_DTYPE))


def _mixed_batch(api, cs, n_cases=20):
    """Constructed cases of every label, and the untouched base instance between them."""
    pick = [c for c in cs.cases if c.kind != "fixed"]
    step = max(1, len(pick) // n_cases)
    part = pick[::step][:n_cases] + [c for c in cs.cases if c.kind == "fixed"][:2]
    return part


def _run(api, torch, path, sol, arrays, n_obs, x_init, ncu):
    if path == "host":
        R = sol.solve_host(*arrays, x_init=x_init)
        return R
    if path == "device_large":
        n = len(arrays[0])
        reps = ncu // n + 2
        hdr, rows, off, sfc = arrays
        big = (np.concatenate([hdr] * reps), np.concatenate([rows] * reps), np.arange(n * reps + 1, dtype=np.uint64) * np.uint64(len(rows) // n),
               np.concatenate([sfc] * reps))
        R = _solve_device(api, torch, sol, big, n_obs)
        for r in range(1, reps):  # every copy answers alike
            for k in ("x", "obj", "status", "info"):
                assert R[k][r * n:(r + 1) * n].tobytes() == R[k][:n].tobytes()
        return {k: v[:n] for k, v in R.items()}
    return _solve_device(api, torch, sol, arrays, n_obs, x_init)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_prescreen_in_front_of_the_solve(api, torch_cuda, path):
    torch = torch_cuda
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    cs = PC.build(api, "generic" if path == "m9" else "c1")
    kw = {}
    if path == "as_only":
        kw["active_set"] = api.ACTIVE_SET_ONLY
    if path == "f32":
        kw["row_format"] = api.ROWS_F32
    part = _mixed_batch(api, cs)
    arrays = PC.to_batch(api, part, cs.n_obs, cs.M)
    n = len(part)
    x_init = None
    if path in ("host", "as_only"):  # a start of the caller's: a fired instance returns it
        rng = np.random.default_rng(3)
        P = cs.ci.P
        x_init = np.concatenate([np.repeat(np.asarray(c.inst.hdr["p0"], float)[:cs.dim], P) for c in part]).reshape(n, -1) + 1e-3 * rng.standard_normal((n, cs.dim * P))

    def handle():
        s = api.Solver(cs.desc(api, **kw))
        if path == "as_off":
            s.set_knob("active_set_off", 1)
        return s

    off_sol, on_sol = handle(), handle()
    cert, _, _ = _certs(api, torch, on_sol, arrays, cs.n_obs)
    assert cert["fired"].sum() >= 5 and (~cert["fired"].astype(bool)).sum() >= 5
    R_off = _run(api, torch, path, off_sol, arrays, cs.n_obs, x_init, ncu)
    on_sol.set_prescreen(api.PRESCREEN_ON)
    assert on_sol.prescreen() == api.PRESCREEN_ON
    R_on = _run(api, torch, path, on_sol, arrays, cs.n_obs, x_init, ncu)
    P = cs.ci.P
    for q, (c, ct) in enumerate(zip(part, cert)):
        if ct["fired"]:
            inf = R_on["info"][q]
            assert R_on["status"][q] == api.STATUS_INFEASIBLE, (q, c.kind, c.s, R_on["status"][q])
            assert inf["flags"] == api.INFO_ACTIVE_SET | api.INFO_PRESCREENED and inf["iterations"] == 0
            assert inf["res_primal"] == ct["violation"] and inf["res_dual"] == 0.0 and inf["gap"] == 0.0 and R_on["obj"][q] == 0.0
            start = x_init[q] if x_init is not None else np.repeat(np.asarray(c.inst.hdr["p0"], float)[:cs.dim], P)
            assert np.array_equal(R_on["x"][q], start)
        else:
            for k in ("x", "obj", "status", "info"):
                assert R_on[k][q].tobytes() == R_off[k][q].tobytes(), (path, q, c.kind, c.s, k, R_on["status"][q], R_off["status"][q])
            assert not (R_on["info"][q]["flags"] & api.INFO_PRESCREENED)
    # ON then OFF: the handle is what one never touched is
    on_sol.set_prescreen(api.PRESCREEN_OFF)
    R_back = _run(api, torch, path, on_sol, arrays, cs.n_obs, x_init, ncu)
    for k in ("x", "obj", "status", "info"):
        assert R_back[k].tobytes() == R_off[k].tobytes(), k


@pytest.mark.gpu
def test_prescreen_on_a_batch_without_an_infeasible_instance_changes_nothing(api, torch_cuda):
    torch = torch_cuda
    from lsc_dr_planner_amd import synth

    M, dim, n_obs = F.SHAPES["c1"]
    sw = synth.Swarm(16, M=M, dim=dim, n_obs=n_obs, seed=5)
    arrays = api.batch_from_swarm(sw.build(), sw.n_obs, M)
    desc = dict(M=M, dim=dim, world_min=sw.world_min, world_max=sw.world_max)
    ref = _solve_device(api, torch, api.Solver(api.make_desc(**desc)), arrays, n_obs)
    assert (ref["status"] == api.STATUS_OPTIMAL).all()
    sol = api.Solver(api.make_desc(**desc))
    sol.set_prescreen(api.PRESCREEN_ON)
    got = _solve_device(api, torch, sol, arrays, n_obs)
    host = sol.solve_host(*arrays)
    assert not sol.prescreen_host(*arrays)["fired"].any()
    for k in ("x", "obj", "status", "info"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert np.array_equal(host["status"], ref["status"]) and np.array_equal(host["x"], ref["x"])


@pytest.mark.gpu
def test_prescreen_refuses_the_lean_form_of_the_phase(api, torch_cuda):
    torch = torch_cuda
    cs = PC.build(api, "c1")
    arrays = PC.to_batch(api, cs.cases[:8], cs.n_obs, cs.M)
    sol = api.Solver(cs.desc(api))
    sol.set_knob("das_screen", 1)
    _solve_device(api, torch, sol, arrays, cs.n_obs)  # (the knob alone is fine)
    sol.set_prescreen(api.PRESCREEN_ON)
    with pytest.raises(api.LscqpError) as e:
        _solve_device(api, torch, sol, arrays, cs.n_obs)
    assert e.value.code == api.ERR_UNSUPPORTED
    sol.set_knob("das_screen", -1)
    assert (_solve_device(api, torch, sol, arrays, cs.n_obs)["status"] >= 0).all()
