"""What dynamic obstacles cost in the replan chain (include/lscqp.h, "dynamic obstacles in the chain"), and that a plan without them costs
what it did.

    python tools/obstacle_timing.py [--repeats 7] [--replans 60] [--mode lsc|clsc] [--plain-only] [--out FILE.json]

Graph replay time per replan, the method of tools/record_timing.py: each repeat resets the plan, warms it up (the eager first replan and two
replays) and times `--replans` replays between two device synchronisations; the plans of a pair alternate within a repeat and the median
over the repeats is reported with the spread.  Two classes:
  forest10   the forest10 world (10 agents, M = 10, 2-D, LSC rows, the device's waypoint decision), 11 row slots, a straight obstacle and a
             patrol in the mission's plane
  room3d     the scenario of tests/test_obstacles_plan_gpu.py (6 agents, M = 5, 3-D, static goals), 7 row slots, its two obstacles
each flown by a plan with the obstacles and by the same plan without them.  --plain-only times the plans without obstacles alone: run it
with LSCQP_LIB naming another build of the library (the parent commit's) in fresh processes, alternating, to compare the two builds.
--mode: the plans' constraint mode, and with it the generator of the obstacle rows: lsc (generateLSC's, the default) or clsc (the plans fly
GEN_CLSC and the obstacles get generateCLSC's rows, lscqp_generate_obstacle_rows_device; room3d then keeps its static goals).
--kernels: instead of the plans, the two obstacle-row kernels alone at the two classes' launch shapes (agents x 2 obstacles x M units), 400
launches back to back between two events each: what the rows node itself takes, apart from what other rows do to the QP behind it.
Prints one JSON line; needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def forest10(api, mode):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
    n, z = len(g["starts"]), float(g["z_2d"])
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    ag = np.zeros(n, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = g["radius"], 2.0, 1.0, 2.0, 1.0

    def plan():
        return api.Plan(sol, wmap, n, n - 1 + 2, ag, constraint_mode=mode, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True, z_2d=z,
                        safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT)

    lo, hi = np.array(g["world_min"]), np.array(g["world_max"])
    c = 0.5 * (lo + hi)
    specs = [dict(type="straight", start=[lo[0] + 0.5, c[1], z], goal=[hi[0] - 0.5, c[1] + 0.5, z], size=0.3, speed=0.3, max_acc=0.5, downwash=1.0),
             dict(type="patrol", waypoints=[[c[0], lo[1] + 0.5, z], [c[0] + 1.0, hi[1] - 0.5, z], [c[0] - 1.0, c[1], z]], size=0.25, speed=0.4, max_acc=0.5,
                  downwash=1.0)]
    return plan, specs, np.array(g["starts"], float), np.array(g["goals"], float), (sol, wmap)


def room3d(api, mode):
    from tests import test_obstacles_plan_gpu as T

    W = T.world()
    sol = T.make_solver(api, W)
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])

    def plan():
        return api.Plan(sol, wmap, T.N, T.N_OBS, T.agents(api, T.N), constraint_mode=mode, sfc_mode=api.SFC_FROM_POINT, optimize_goal=False,
                        closed_loop=True, safety_samples=2, record_time_step=0.1)

    return plan, T.obstacle_specs(), W["starts"], W["goals"], (sol, wmap)


def measure(api, torch, make, repeats, replans, plain_only, mode):
    plan, specs, starts, goals, keep = make(api, mode)
    plans = {"without": plan()}
    if not plain_only:
        plans["with"] = plan()
        plans["with"].set_obstacles(api.obstacle_models(specs))
    times = {k: [] for k in plans}
    names = list(plans)
    for rep in range(repeats):
        for name in (names if rep % 2 == 0 else names[::-1]):
            p = plans[name]
            p.reset(starts, goals)
            for _ in range(3):
                p.step(graph=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(replans):
                p.step(graph=True)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / replans * 1e6)
    out = dict(agents=len(starts))
    for name, p in plans.items():
        out["us_" + name] = statistics.median(times[name])
        out["spread_" + name] = [min(times[name]), max(times[name])]
        out["nodes_" + name] = p.graph_nodes()
        out["qp_failed_" + name] = int((p.get(api.PLAN_STATUS) != 0).sum())
    if not plain_only:
        out["obstacles_us"] = out["us_with"] - out["us_without"]
    for p in plans.values():
        p.close()
    keep[1].close()
    keep[0].close()
    return out


def kernels(api, torch, launches=400, repeats=5):
    """us per launch of lscqp_generate_obstacle_rows_device in both modes, per class shape (random agents 1 .. 3 m from moving obstacles)"""
    dev, out = torch.device("cuda", 0), {}
    rng = np.random.default_rng(0)
    par = api.ObstacleParam(1.0, 0.75, 3.0, 0.1, 1, 1)
    for name, (M, dim, n) in (("forest10", (10, 2, 10)), ("room3d", (5, 3, 6))):
        sol = api.Solver(api.make_desc(M=M, dim=dim, dt=0.2, world_min=(-40, -40, -40), world_max=(40, 40, 40)))
        table = np.zeros(2, api.OBSTACLE_DTYPE)
        table["position"], table["velocity"] = np.float32(rng.uniform(-3, 3, (2, 3))), np.float32(rng.uniform(-0.3, 0.3, (2, 3)))
        table["radius"], table["downwash"], table["max_acc"] = 0.25, 1.0, 1.0
        traj = np.float32(rng.uniform(4, 8, (n, 1, 1, 3)) + rng.uniform(-0.3, 0.3, (n, M, 6, 3))).astype(np.float64)
        if dim == 2:
            table["position"][:, 2], table["velocity"][:, 2], traj[..., 2] = 1.0, 0.0, 1.0
        hdr = np.zeros(n, api.HEADER_DTYPE)
        hdr["amax"] = 2.0
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        t = [up(traj), up(np.tile(np.arange(2, dtype=np.int32), n)), up(table), None, up(np.full(n, 0.15)), up(traj[:, M - 1, 5] + 1.0), up(hdr)]
        rows = torch.zeros(n * 2 * M * 6 * 4, dtype=torch.float64, device=dev)
        res = {}
        for mode, tag in ((api.GEN_LSC, "lsc"), (api.GEN_CLSC, "clsc")):
            go = lambda: sol.generate_obstacle_rows_device(mode, par, n, 2, 0, *t, rows, 2, 0)  # noqa: E731
            times = []
            for _ in range(repeats):
                for _ in range(20):
                    go()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    go()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / launches)
            res["us_" + tag] = statistics.median(times)
            res["spread_" + tag] = [min(times), max(times)]
        out[name] = dict(units=n * 2 * M, **res)
        sol.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--replans", type=int, default=60)
    ap.add_argument("--plain-only", action="store_true", help="only the plans without obstacles (any build of the library: LSCQP_LIB)")
    ap.add_argument("--mode", default="lsc", choices=("lsc", "clsc"), help="the plans' constraint mode: whose rows the obstacles get")
    ap.add_argument("--kernels", action="store_true", help="the two obstacle-row kernels alone at the classes' launch shapes")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    assert torch.cuda.is_available(), "obstacle_timing.py measures on the GPU"
    mode = api.GEN_CLSC if a.mode == "clsc" else api.GEN_LSC
    if a.kernels:
        res = dict(lib=os.path.basename(api.LIB_PATH), kernels=kernels(api, torch))
    else:
        res = dict(lib=os.path.basename(api.LIB_PATH), mode=a.mode, plain_only=a.plain_only, repeats=a.repeats, replans=a.replans,
                   forest10=measure(api, torch, forest10, a.repeats, a.replans, a.plain_only, mode),
                   room3d=measure(api, torch, room3d, a.repeats, a.replans, a.plain_only, mode))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    print(line)
