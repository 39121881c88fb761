"""What dynamic obstacles cost in the replan chain (include/lscqp.h, "dynamic obstacles in the chain"), and that a plan without them costs
what it did.

    python tools/obstacle_timing.py [--repeats 7] [--replans 60] [--plain-only] [--out FILE.json]

Graph replay time per replan, the method of tools/record_timing.py: each repeat resets the plan, warms it up (the eager first replan and two
replays) and times `--replans` replays between two device synchronisations; the plans of a pair alternate within a repeat and the median
over the repeats is reported with the spread.  Two classes:
  forest10   the forest10 world (10 agents, M = 10, 2-D, LSC rows, the device's waypoint decision), 11 row slots, a straight obstacle and a
             patrol in the mission's plane
  room3d     the scenario of tests/test_obstacles_plan_gpu.py (6 agents, M = 5, 3-D, static goals), 7 row slots, its two obstacles
each flown by a plan with the obstacles and by the same plan without them.  --plain-only times the plans without obstacles alone: run it
with LSCQP_LIB naming another build of the library (the parent commit's) in fresh processes, alternating, to compare the two builds.
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


def forest10(api):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
    n, z = len(g["starts"]), float(g["z_2d"])
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    ag = np.zeros(n, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = g["radius"], 2.0, 1.0, 2.0, 1.0

    def plan():
        return api.Plan(sol, wmap, n, n - 1 + 2, ag, constraint_mode=api.GEN_LSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True, z_2d=z,
                        safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT)

    lo, hi = np.array(g["world_min"]), np.array(g["world_max"])
    c = 0.5 * (lo + hi)
    specs = [dict(type="straight", start=[lo[0] + 0.5, c[1], z], goal=[hi[0] - 0.5, c[1] + 0.5, z], size=0.3, speed=0.3, max_acc=0.5, downwash=1.0),
             dict(type="patrol", waypoints=[[c[0], lo[1] + 0.5, z], [c[0] + 1.0, hi[1] - 0.5, z], [c[0] - 1.0, c[1], z]], size=0.25, speed=0.4, max_acc=0.5,
                  downwash=1.0)]
    return plan, specs, np.array(g["starts"], float), np.array(g["goals"], float), (sol, wmap)


def room3d(api):
    from tests import test_obstacles_plan_gpu as T

    W = T.world()
    sol = T.make_solver(api, W)
    wmap = api.WorldMap(W["boxes"], W["world_min"], W["world_max"], W["resolution"], W["max_dist"])
    return (lambda: T.make_plan(api, sol, wmap)), T.obstacle_specs(), W["starts"], W["goals"], (sol, wmap)


def measure(api, torch, make, repeats, replans, plain_only):
    plan, specs, starts, goals, keep = make(api)
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--replans", type=int, default=60)
    ap.add_argument("--plain-only", action="store_true", help="only the plans without obstacles (any build of the library: LSCQP_LIB)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    assert torch.cuda.is_available(), "obstacle_timing.py measures on the GPU"
    res = dict(lib=os.path.basename(api.LIB_PATH), plain_only=a.plain_only, repeats=a.repeats, replans=a.replans,
               forest10=measure(api, torch, forest10, a.repeats, a.replans, a.plain_only), room3d=measure(api, torch, room3d, a.repeats, a.replans, a.plain_only))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    print(line)
