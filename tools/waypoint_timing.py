"""What the waypoint layer costs on the device (include/lscqp.h, "the grid planner / MAPF layer"): HIP events around single launches,
>= 200 repeats after warm-up, medians; whole-replan times from fresh processes, interleaved.

    python tools/waypoint_timing.py --part kernels                  fields at reset and the decision per replan, by agent count and grid size
    python tools/waypoint_timing.py --part chain --agents 0|64      one process: the replan chain, eager and graph (--mode 0|1; --tree DIR takes
                                                                    lsc_dr_planner_amd from another checkout, e.g. the parent commit's, mode 0)
    python tools/waypoint_timing.py --part closed_loop              tools/closed_loop.py per replan with router=host and router=device
    python tools/waypoint_timing.py --part chains --agents 0|64 [--parent DIR] [--runs 5]
                                                                    the driver of `chain`: fresh child processes, parent mode 0 / mode 0 / mode 1
                                                                    (and parent mode 1) interleaved, medians and the run-to-run spread of each
    python tools/waypoint_timing.py --part missions --missions K [--tree DIR]
                                                                    one process: K copies of forest10 as K plans stepped one after another
                                                                    and (this checkout) as ONE plan with K missions, graph replay
    python tools/waypoint_timing.py --part missions_sweep [--missions-list 1,8,25] [--parent DIR] [--runs 5]
                                                                    the driver of `missions`: fresh child processes, interleaved
    python tools/waypoint_timing.py --part decision --missions K    the decision alone: one workgroup per mission against the single-workgroup
                                                                    decision over the same 10 K agents
    python tools/waypoint_timing.py --part decision_wide [--agents-list 10,64,512,4096]
                                                                    lscqp_waypoints_device against lscqp_waypoints_wide_device on the 201 x 201
                                                                    grid at ranges -1, 3, 2, 1 m: same inputs, outputs compared equal first,
                                                                    then timed in the same process, interleaved
    --decision 0|1|2 with --part chain / chains (mode 1)            the plan's lscqp_plan_set_waypoint_decision; chains adds a mode-1 WIDE variant

Every part prints JSON lines; profiles/r09_waypoints.txt, profiles/r10_missions.txt and profiles/r12_waypoints_wide.txt are transcripts."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _forest(side, n_boxes, seed=0):
    rng = np.random.default_rng(seed)
    half = side / 2
    boxes = [[c[0], c[1], 0.5, 0.5, 0.5, 1.0] for c in rng.uniform(-half + 1, half - 1, (n_boxes, 2))]
    return {"boxes": boxes, "world_min": [-half, -half, 0.0], "world_max": [half, half, 1.0], "resolution": 0.1, "max_dist": 1.0, "z_2d": 0.6, "radius": 0.15}


def _free_nodes(occ, gmin, n, seed, distinct):
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(~occ.astype(bool))
    pick = rng.choice(len(xs), size=n, replace=not distinct)
    return np.c_[gmin[0] + 0.5 * xs[pick], gmin[1] + 0.5 * ys[pick], np.full(n, 0.6)]


def _events(torch, fn, repeats, warmup, before=None):
    for _ in range(warmup):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    for a, b in ev:
        if before:
            before()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    return dict(median_us=float(np.median(t)), p10_us=float(np.percentile(t, 10)), p90_us=float(np.percentile(t, 90)), repeats=repeats)


def part_kernels(a):
    import torch

    from lsc_dr_planner_amd import api

    dev = torch.device("cuda", 0)
    up = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)  # noqa: E731
    f10 = json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
    worlds = [("21x21", f10), ("201x201", _forest(100.0, 3000))]
    for gname, w in worlds:
        wmap = api.WorldMap(w["boxes"], w["world_min"], w["world_max"], w["resolution"], w["max_dist"])
        grid = api.Grid(wmap, 0.5, w["radius"], w["z_2d"])
        occ = grid.download()
        nfree = int((occ == 0).sum())
        for n in (10, 64, 512, 4096):
            if gname == "21x21" and n == 10:
                starts, goals = np.array(f10["starts"], float), np.array(f10["goals"], float)
            else:
                distinct = n <= nfree // 2
                starts, goals = _free_nodes(occ, grid.grid_min, n, 1, distinct), _free_nodes(occ, grid.grid_min, n, 2, False)
            d_s, d_g = up(starts), up(goals)
            d_field = torch.empty((n, int(grid.dims[1]), int(grid.dims[0])), dtype=torch.int32, device=dev)
            d_init = torch.empty(n, dtype=torch.int32, device=dev)
            r = _events(torch, lambda: grid.fields(d_s, d_g, d_field, d_init), a.repeats, 20)
            print(json.dumps(dict(what="fields", grid=gname, agents=n, max_init_d=int(d_init[d_init < api.GRID_UNREACHABLE].max().item()), **r)), flush=True)
            if not (n <= nfree // 2):
                continue  # (the decision needs distinct waypoint nodes: 4096 agents do not fit a 21 x 21 grid)
            st = np.zeros((n, 9))
            st[:, :3] = starts
            M = 10
            x = np.repeat(starts[:, :2, None], M * 6, axis=2).reshape(n, -1)  # hover plans
            d_st, d_x, d_cg, d_way0 = up(st), up(x), up(np.float32(starts).astype(float)), up(np.float32(starts).astype(float))
            d_way = d_way0.clone()
            for rng_name, rng in (("one group", -1.0), ("range 3 m", 3.0), ("range 1 m", 1.0)):
                grid.reserve(n)
                g, _, u = grid.waypoints(rng, M, 2, d_st, d_x, d_cg, d_field, d_init, d_way)
                torch.cuda.synchronize()
                groups, moved = int(torch.unique(g).numel()), int(u.sum().item())
                r = _events(torch, lambda: grid.waypoints(rng, M, 2, d_st, d_x, d_cg, d_field, d_init, d_way), a.repeats, 20, before=lambda: d_way.copy_(d_way0))
                assert grid.status() == 0
                print(json.dumps(dict(what="decision", grid=gname, agents=n, range=rng_name, groups=groups, waypoints_moved=moved, **r)), flush=True)
        grid.close()
        wmap.close()


def part_chain(a):
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    from lsc_dr_planner_amd import api  # (before closed_loop, which puts this checkout in front of --tree)

    import closed_loop

    W = closed_loop.random_forest_world(a.agents) if a.agents > 0 else json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
    N = len(W["starts"])
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    n_obs = min(N - 1, sol.max_obstacles())
    ag = np.zeros(N, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = W["radius"], 2.0, 1.0, 2.0, 1.0
    kw = dict(waypoint_mode=1) if a.mode == 1 else {}
    plan = api.Plan(sol, wmap, N, n_obs, ag, constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, closed_loop=True, z_2d=W["z_2d"], **kw)
    if a.decision:
        plan.set_waypoint_decision(a.decision)
    router = closed_loop.GridRouter(W, wmap.download()[0], wmap.key0) if a.mode == 0 else None
    starts, desired = np.array(W["starts"], dtype=np.float64), np.array(W["goals"], dtype=np.float64)
    # (host wall time around step + synchronise, the figure a caller feels; the kernels part uses device events)
    out = dict(what="chain", clock="host wall time around step + synchronize", agents=N, mode=a.mode, decision=a.decision, lib=os.path.dirname(api.__file__), steps=a.steps)
    for form in ("eager", "graph"):
        plan.reset(starts, desired) if a.mode == 1 else plan.reset(starts)
        way = starts.copy()
        t_dev, failed = [], 0
        for k in range(a.steps):
            if a.mode == 0:  # (the host router of tools/closed_loop.py between replans; its time is not in the figure)
                state = plan.get(api.PLAN_STATE).reshape(N, 9)
                for i in range(N):
                    if np.abs(state[i, :2] - way[i, :2]).max() < 0.3:
                        way[i, :2] = router.next_waypoint(way[i], desired[i])[0]
                plan.put(api.PLAN_WAYPOINT, np.float32(way).astype(np.float64))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            plan.step(graph=(form == "graph"))
            torch.cuda.synchronize()
            if k >= 3:
                t_dev.append(time.perf_counter() - t1)
            failed += int((plan.get(api.PLAN_STATUS) != 0).sum())
        state = plan.get(api.PLAN_STATE).reshape(N, 9)
        out[form + "_us"] = float(np.median(t_dev) * 1e6)
        out[form + "_failed_qps"] = failed
        out[form + "_progress_m"] = float((np.linalg.norm(desired[:, :2] - starts[:, :2], axis=1) - np.linalg.norm(desired[:, :2] - state[:, :2], axis=1)).mean())
    out["graph_nodes"] = plan.graph_nodes()
    print(json.dumps(out), flush=True)


def part_chains(a):
    me = os.path.abspath(__file__)
    variants = [("mode0", ["--mode", "0"]), ("mode1", ["--mode", "1"]), ("mode1_wide", ["--mode", "1", "--decision", "1"])]
    if a.parent:
        variants = [("parent_mode0", ["--mode", "0", "--tree", a.parent]), variants[0], ("parent_mode1", ["--mode", "1", "--tree", a.parent]), variants[1], variants[2]]
    res = {k: [] for k, _ in variants}
    for _ in range(a.runs):
        for name, extra in variants:  # interleaved: one run of each, then the next round
            r = subprocess.run([sys.executable, me, "--part", "chain", "--agents", str(a.agents), "--steps", str(a.steps)] + extra, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                raise SystemExit("child failed (%s): nothing more is started" % name)
            res[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    for name, rows in res.items():
        for form in ("eager", "graph"):
            v = [r[form + "_us"] for r in rows]
            print(json.dumps(dict(what="chains", clock="host wall time around step + synchronize, median of %d replans per run" % (a.steps - 3), agents=rows[0]["agents"], variant=name, form=form, runs_us=[round(x, 1) for x in v], median_us=round(float(np.median(v)), 1),
                                  spread_us=round(max(v) - min(v), 1), graph_nodes=rows[0]["graph_nodes"], failed_qps=sum(r[form + "_failed_qps"] for r in rows),
                                  progress_m=round(rows[0][form + "_progress_m"], 2))), flush=True)


def part_missions(a):
    """K copies of forest10.  `separate`: K plans of ten agents (what a caller without the partition runs), every plan's graph launched
    one after another, one wait at the end.  `batched`: one plan with K missions.  Host wall time per replan of ALL K missions."""
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    from lsc_dr_planner_amd import api

    W = json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
    K, n = a.missions, len(W["starts"])
    starts, goals = np.array(W["starts"], dtype=np.float64), np.array(W["goals"], dtype=np.float64)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=W["world_min"], world_max=W["world_max"]))
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])

    def make(N, **kw):
        ag = np.zeros(N, api.AGENT_PARAM_DTYPE)
        ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = W["radius"], 2.0, 1.0, 2.0, 1.0
        return api.Plan(sol, wmap, N, n - 1, ag, constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, closed_loop=True, z_2d=W["z_2d"], waypoint_mode=1, **kw)

    def fly(plans):
        t, failed = [], 0
        for k in range(a.steps):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for p in plans:
                p.step(graph=True)
            torch.cuda.synchronize()
            if k >= 3:
                t.append(time.perf_counter() - t1)
            failed += sum(int((p.get(api.PLAN_STATUS) != 0).sum()) for p in plans)
        return float(np.median(t) * 1e6), failed

    out = dict(what="missions", clock="host wall time around the steps of all K missions + synchronize", missions=K, agents=K * n, lib=os.path.dirname(api.__file__),
               steps=a.steps)
    plans = [make(n) for _ in range(K)]
    for p in plans:
        p.reset(starts, goals)
    out["separate_us"], out["separate_failed_qps"] = fly(plans)
    for p in plans:
        p.close()
    if hasattr(api.Plan, "set_missions"):
        plan = make(K * n, mission_offsets=np.arange(K + 1) * n)
        plan.reset(np.tile(starts, (K, 1)), np.tile(goals, (K, 1)))
        out["batched_us"], out["batched_failed_qps"] = fly([plan])
        out["graph_nodes"] = plan.graph_nodes()
        plan.close()
    print(json.dumps(out), flush=True)


def part_missions_sweep(a):
    me = os.path.abspath(__file__)
    for K in [int(v) for v in a.missions_list.split(",")]:
        variants = [("this", [])] + ([("parent", ["--tree", a.parent])] if a.parent else [])
        res = {k: [] for k, _ in variants}
        for _ in range(a.runs):
            for name, extra in variants:
                r = subprocess.run([sys.executable, me, "--part", "missions", "--missions", str(K), "--steps", str(a.steps)] + extra, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                    raise SystemExit("child failed (%s, K = %d): nothing more is started" % (name, K))
                res[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
        for name, rows in res.items():
            for form in ("separate", "batched"):
                if form + "_us" not in rows[0]:
                    continue
                v = [r[form + "_us"] for r in rows]
                print(json.dumps(dict(what="missions_sweep", clock=rows[0]["clock"] + ", median of %d replans per run" % (a.steps - 3), missions=K, agents=rows[0]["agents"],
                                      lib=name, form=form, runs_us=[round(x, 1) for x in v], median_us=round(float(np.median(v)), 1), spread_us=round(max(v) - min(v), 1),
                                      failed_qps=sum(r[form + "_failed_qps"] for r in rows))), flush=True)


def part_decision(a):
    """The decision alone on a 40 m forest (81 x 81 nodes, tables in LDS): K missions of ten agents as one workgroup per mission, and the
    same 10 K agents as one swarm in the single workgroup."""
    import torch

    from lsc_dr_planner_amd import api

    dev = torch.device("cuda", 0)
    up = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)  # noqa: E731
    w = _forest(40.0, 300)
    wmap = api.WorldMap(w["boxes"], w["world_min"], w["world_max"], w["resolution"], w["max_dist"])
    grid = api.Grid(wmap, 0.5, w["radius"], w["z_2d"])
    occ = grid.download()
    K, per = a.missions, 10
    n = K * per
    off = np.arange(K + 1) * per
    starts, goals = _free_nodes(occ, grid.grid_min, n, 1, True), _free_nodes(occ, grid.grid_min, n, 2, False)
    d_s, d_g, d_off = up(starts), up(goals), up(off, np.int64)
    st = np.zeros((n, 9))
    st[:, :3] = starts
    x = np.repeat(starts[:, :2, None], 60, axis=2).reshape(n, -1)  # hover plans
    d_st, d_x, d_cg, d_way0 = up(st), up(x), up(np.float32(starts).astype(float)), up(np.float32(starts).astype(float))
    d_way = d_way0.clone()
    for rng_name, rng in (("one group per mission / swarm", -1.0), ("range 3 m", 3.0)):
        d_field, d_init = grid.fields(d_s, d_g)
        g, _, u = grid.waypoints(rng, 10, 2, d_st, d_x, d_cg, d_field, d_init, d_way)
        torch.cuda.synchronize()
        r = _events(torch, lambda: grid.waypoints(rng, 10, 2, d_st, d_x, d_cg, d_field, d_init, d_way), a.repeats, 20, before=lambda: d_way.copy_(d_way0))
        print(json.dumps(dict(what="decision", form="one swarm, one workgroup", agents=n, range=rng_name, groups=int(torch.unique(g).numel()), waypoints_moved=int(u.sum().item()), **r)), flush=True)
        d_field, d_init = grid.fields_missions(off, d_s, d_g, d_offsets=d_off)
        d_way.copy_(d_way0)
        g, _, u = grid.waypoints_missions(off, rng, 10, 2, d_st, d_x, d_cg, d_field, d_init, d_way, d_offsets=d_off)
        torch.cuda.synchronize()
        r = _events(torch, lambda: grid.waypoints_missions(off, rng, 10, 2, d_st, d_x, d_cg, d_field, d_init, d_way, d_offsets=d_off), a.repeats, 20,
                    before=lambda: d_way.copy_(d_way0))
        assert not grid.mission_status(K).any() and grid.status() == 0
        print(json.dumps(dict(what="decision", form="%d missions, one workgroup each" % K, agents=n, range=rng_name, groups=int(torch.unique(g).numel()), waypoints_moved=int(u.sum().item()), **r)), flush=True)
    grid.close()
    wmap.close()


def part_decision_wide(a):
    """The one-workgroup decision and the wide one on the 201 x 201 grid of `kernels`, same inputs: hover plans at distinct free nodes.  Per
    agent count and range the outputs of the two are compared equal first; then `rounds` rounds of (repeats / rounds one-workgroup calls,
    repeats / rounds wide calls) are timed with HIP events, and the medians are over all of a form's calls."""
    import torch

    from lsc_dr_planner_amd import api

    dev = torch.device("cuda", 0)
    up = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)  # noqa: E731
    w = _forest(100.0, 3000)
    wmap = api.WorldMap(w["boxes"], w["world_min"], w["world_max"], w["resolution"], w["max_dist"])
    grid = api.Grid(wmap, 0.5, w["radius"], w["z_2d"])
    occ = grid.download()
    M, rounds = 10, 4
    for n in [int(v) for v in a.agents_list.split(",")]:
        starts, goals = _free_nodes(occ, grid.grid_min, n, 1, True), _free_nodes(occ, grid.grid_min, n, 2, False)
        d_field, d_init = grid.fields(up(starts), up(goals))
        st = np.zeros((n, 9))
        st[:, :3] = starts
        x = np.repeat(starts[:, :2, None], M * 6, axis=2).reshape(n, -1)  # hover plans
        d_st, d_x, d_cg, d_way0 = up(st), up(x), up(np.float32(starts).astype(float)), up(np.float32(starts).astype(float))
        d_way = d_way0.clone()
        grid.reserve_wide(n)
        forms = (("one_workgroup", grid.waypoints), ("wide", grid.waypoints_wide))
        for rng in (-1.0, 3.0, 2.0, 1.0):
            outs = {}
            for name, fn in forms:
                d_way.copy_(d_way0)
                g, d, u = fn(rng, M, 2, d_st, d_x, d_cg, d_field, d_init, d_way)
                torch.cuda.synchronize()
                outs[name] = (g.clone(), d.clone(), u.clone(), d_way.clone())
            assert grid.status() == 0
            assert all(torch.equal(p, q) for p, q in zip(outs["one_workgroup"], outs["wide"])), "the two forms disagree: nothing is timed"
            g, _, u, _ = outs["wide"]
            sizes = torch.bincount(g.long())
            t = {name: [] for name, _ in forms}
            per = max(1, a.repeats // rounds)
            for _ in range(rounds):  # interleaved
                for name, fn in forms:
                    r = _events(torch, lambda: fn(rng, M, 2, d_st, d_x, d_cg, d_field, d_init, d_way), per, 5, before=lambda: d_way.copy_(d_way0))
                    t[name].append(r["median_us"])
            row = dict(what="decision_wide", grid="201x201", agents=n, range=rng, groups=int((sizes > 0).sum().item()), groups_walked=int((sizes > 1).sum().item()),
                       largest_group=int(sizes.max().item()), waypoints_moved=int(u.sum().item()), calls_per_form=per * rounds)
            for name, _ in forms:
                row[name + "_us"] = round(float(np.median(t[name])), 1)
                row[name + "_rounds_us"] = [round(v, 1) for v in t[name]]
            row["one_over_wide"] = round(row["one_workgroup_us"] / row["wide_us"], 2)
            print(json.dumps(row), flush=True)
    grid.close()
    wmap.close()


def part_closed_loop(a):
    import closed_loop

    world = os.path.join(ROOT, "tests", "golden", "forest10_world.json")
    closed_loop.run(world, steps=5)  # (code objects, the first import of torch)
    for router in ("host", "device", "host", "device"):
        t0 = time.perf_counter()
        closed_loop.run(world, steps=10, router=router)
        t1 = time.perf_counter()
        log = closed_loop.run(world, steps=60, router=router)
        t2 = time.perf_counter()
        # (the two runs share their set-up -- map, corridors, the router's grid --, so the difference is 50 replans)
        print(json.dumps(dict(what="closed_loop", router=router, wall_ms_per_replan=round(((t2 - t1) - (t1 - t0)) / 50 * 1e3, 3), run60_s=round(t2 - t1, 3),
                              qp_failed=log["qp_failed"], invalid=log["invalid"], min_safety_ratio=log["min_safety_ratio"], mean_progress_m=round(log["mean_progress_m"], 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=("kernels", "chain", "chains", "closed_loop", "missions", "missions_sweep", "decision", "decision_wide"))
    ap.add_argument("--agents-list", default="10,64,512,4096")
    ap.add_argument("--decision", type=int, default=0)
    ap.add_argument("--missions", type=int, default=25)
    ap.add_argument("--missions-list", default="1,8,25")
    ap.add_argument("--agents", type=int, default=0)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if a.part not in ("chain", "missions") or not a.tree:
        sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    {"kernels": part_kernels, "chain": part_chain, "chains": part_chains, "closed_loop": part_closed_loop, "missions": part_missions,
     "missions_sweep": part_missions_sweep, "decision": part_decision, "decision_wide": part_decision_wide}[a.part](a)


if __name__ == "__main__":
    main()
