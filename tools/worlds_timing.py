"""What a world per mission costs in the replan chain (include/lscqp.h, "each mission over its own world"), what it saves against one plan per
world, and that a plan without worlds costs what it did.

    python tools/worlds_timing.py --mode plain  [--repeats 5] [--replans 40] [--out FILE]
    python tools/worlds_timing.py --mode worlds [--repeats 5] [--replans 40] [--out FILE]

Graph replay time per replan, the method of tools/obstacle_timing.py: each repeat resets the plan, warms it up (the eager first replan and two
replays) and times `--replans` replays between two device synchronisations; the sides of a pair alternate within a repeat and the median over
the repeats is reported with the spread.
  --mode plain   plans WITHOUT worlds, nothing of the new interface: 25 copies of forest10 in one plan over one map, forest10 alone (10 agents)
                 and the 3-D room of tests/test_obstacles_plan_gpu.py.  Run it in fresh processes, alternating, with LSCQP_LIB naming the parent
                 commit's build and without: the bar is that this tree's median lies inside the parent's own min-max.
  --mode worlds  (b) 25 ten-agent missions in one plan: over one map / over a set that lists that SAME map 25 times (identical work: what the
                 worlds launch itself costs) / over the four fixture worlds repeated (each mission on free nodes of its own world);
                 (c) 30 ten-agent plans stepped in turn, each over its own world, against one plan with 30 missions and 30 worlds.
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


def _agents(api, radius, n):
    ag = np.zeros(n, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = radius, 2.0, 1.0, 2.0, 1.0
    return ag


def _plan(api, sol, wmap, g, n, **kw):
    return api.Plan(sol, wmap, n, 9, _agents(api, g["radius"], n), constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True,
                    z_2d=float(g["z_2d"]), safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT, **kw)


def time_sides(torch, sides, repeats, replans):
    """sides: {name: (plans stepped in turn, starts per plan, goals per plan)} -> {name: (median us per replan of the side, [min, max])}"""
    times = {k: [] for k in sides}
    names = list(sides)
    for rep in range(repeats):
        for name in (names if rep % 2 == 0 else names[::-1]):
            plans, starts, goals = sides[name]
            for p, s, t in zip(plans, starts, goals):
                p.reset(s, t)
                for _ in range(3):
                    p.step(graph=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(replans):
                for p in plans:
                    p.step(graph=True)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / replans * 1e6)
    return {k: (statistics.median(v), [min(v), max(v)]) for k, v in times.items()}


def _report(api, sides, res):
    out = {}
    for name, (plans, _, _) in sides.items():
        out["us_" + name], out["spread_" + name] = res[name]
        out["nodes_" + name] = plans[0].graph_nodes()
        out["qp_failed_" + name] = int(sum((p.get(api.PLAN_STATUS) != 0).sum() for p in plans))
        out["sfc_kept_" + name] = int(sum((p.get(api.PLAN_SFC_STATUS) != 1).sum() for p in plans))
    return out


def plain(api, torch, repeats, replans):
    from tools import obstacle_timing as OT

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
    n, K = len(g["starts"]), 25
    starts, goals = np.array(g["starts"], float), np.array(g["goals"], float)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    out = {}
    for name, plan, s, t in (("missions25", _plan(api, sol, wmap, g, K * n, mission_offsets=np.arange(K + 1) * n), np.tile(starts, (K, 1)), np.tile(goals, (K, 1))),
                             ("forest10", _plan(api, sol, wmap, g, n), starts, goals)):
        sides = {name: ([plan], [s], [t])}
        out.update(_report(api, sides, time_sides(torch, sides, repeats, replans)))
        plan.close()
    make, _, s, t, keep = OT.room3d(api)
    sides = {"room3d": ([make()], [s], [t])}
    out.update(_report(api, sides, time_sides(torch, sides, repeats, replans)))
    sides["room3d"][0][0].close()
    return out


def worlds(api, torch, repeats, replans):
    from tests import world_cases as WLD

    g = WLD.fixture()
    n = 10
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    maps = [api.WorldMap(b, g["world_min"], g["world_max"], g["resolution"], g["max_dist"]) for b in g["worlds"]]
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def mission(k, world):  # ten agents on free nodes of `world`, from k
        p = WLD.free_nodes(g["worlds"][world], 2 * n, [7, k], g)
        return p[:n], p[n:]

    out = dict(compute_units=cus)
    # (b) 25 missions in one plan
    K = 25
    off = np.arange(K + 1) * n
    in0 = [mission(k, 0) for k in range(K)]
    own = [mission(k, k % 4) for k in range(K)]
    cat = lambda ms, j: np.concatenate([m[j] for m in ms])  # noqa: E731
    same_map, four = api.Worlds([maps[0]] * K), api.Worlds([maps[k % 4] for k in range(K)])
    plans = {name: _plan(api, sol, maps[0], g, K * n, mission_offsets=off) for name in ("one_map", "same_map_25_times", "four_worlds_repeated")}
    plans["same_map_25_times"].set_worlds(same_map)
    plans["four_worlds_repeated"].set_worlds(four)
    sides = {"one_map": ([plans["one_map"]], [cat(in0, 0)], [cat(in0, 1)]), "same_map_25_times": ([plans["same_map_25_times"]], [cat(in0, 0)], [cat(in0, 1)]),
             "four_worlds_repeated": ([plans["four_worlds_repeated"]], [cat(own, 0)], [cat(own, 1)])}
    out["b_25_missions"] = _report(api, sides, time_sides(torch, sides, repeats, replans))
    out["b_25_missions"]["corridor_build"] = "throughput" if K * n > cus else "latency"
    for p in plans.values():
        p.close()
    # (c) 30 plans in turn against one plan with 30 missions and 30 worlds
    K = 30
    off = np.arange(K + 1) * n
    own = [mission(k, k % 4) for k in range(K)]
    ws = api.Worlds([maps[k % 4] for k in range(K)])
    one = _plan(api, sol, maps[0], g, K * n, mission_offsets=off)
    one.set_worlds(ws)
    each = [_plan(api, sol, maps[k % 4], g, n) for k in range(K)]
    sides = {"one_plan_30_worlds": ([one], [cat(own, 0)], [cat(own, 1)]), "30_plans_in_turn": (each, [m[0] for m in own], [m[1] for m in own])}
    out["c_30_missions"] = _report(api, sides, time_sides(torch, sides, repeats, replans))
    out["c_30_missions"]["ratio"] = out["c_30_missions"]["us_30_plans_in_turn"] / out["c_30_missions"]["us_one_plan_30_worlds"]
    out["c_30_missions"]["corridor_build"] = {"one_plan_30_worlds": "throughput" if K * n > cus else "latency", "30_plans_in_turn": "latency"}
    one.close()
    for p in each:
        p.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("plain", "worlds"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replans", type=int, default=40)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    assert torch.cuda.is_available(), "worlds_timing.py measures on the GPU"
    res = dict(lib=os.path.basename(api.LIB_PATH), mode=a.mode, repeats=a.repeats, replans=a.replans)
    res.update((plain if a.mode == "plain" else worlds)(api, torch, a.repeats, a.replans))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    print(line)
