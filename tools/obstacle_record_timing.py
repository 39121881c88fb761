"""What the obstacle record costs per replan and what it saves over a whole flight (include/lscqp.h, "the obstacle record").

    python tools/obstacle_record_timing.py [--repeats 5] [--replans 60] [--max 400] [--plain-only] [--out FILE.json]

(a) One replan: graph replay time per replan of forest10 (one mission of 10 agents) and of 25 x forest10 (a partition of 25 missions), each
    with two obstacles (a straight one and a patrol, CLSC rows) and a record -- without the option and with it.  As
    tools/flight_log_timing.py measures the log: each repeat resets the plan, warms it up (the eager first replan and two replays) and times
    `--replans` replays between two device synchronisations; the two plans alternate within a repeat; the median over the repeats and the
    spread are reported.  --plain-only times the plan without the option alone and calls nothing of the obstacle record, so that LSCQP_LIB
    may name a library that predates it (an A/B against the parent commit, in fresh processes).
(b) Whole flights: 25 seeded missions over the forest10 world with the two obstacles, flown to the finish (or --max replans) by
    lscqp_plan_run (check_every 16) with the obstacle record, the figures downloaded behind the flight -- against the stepped loop that is
    the other way to the same number: one graph replay, a synchronisation and a download of LSCQP_PLAN_OBS_SAFETY and of the records per
    replan, the minimum kept on the host for every mission not yet finished.  Both must arrive at the same safety_ratio_obs per mission, bit
    for bit.
Prints a table and one JSON line; needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from record_timing import _plan  # noqa: E402

N_DYN = 2


def obstacle_specs(z):
    return [dict(type="straight", start=[2.0, -1.0, z], goal=[-2.0, 1.0, z], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0),
            dict(type="patrol", waypoints=[[-2.5, -1.5, z], [2.5, -1.5, z]], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0)]


def one_replan(api, torch, g, copies, repeats, replans, plain_only):
    n = len(g["starts"])
    starts, goals = np.tile(np.array(g["starts"], float), (copies, 1)), np.tile(np.array(g["goals"], float), (copies, 1))
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    off = np.arange(copies + 1) * n if copies > 1 else None
    models = api.obstacle_models(obstacle_specs(float(g["z_2d"])))
    names = ("plain",) if plain_only else ("plain", "obstacle_record")
    plans = {k: _plan(api, sol, wmap, g, copies * n, n - 1 + N_DYN, off) for k in names}
    for k, p in plans.items():
        p.set_obstacles(models)
        p.set_record(1e-3)  # (never reached within the window: every node works in every replan)
        if k == "obstacle_record":
            p.set_obstacle_record()
    times = {k: [] for k in plans}
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
    out = dict(agents=copies * n, missions=copies, nodes={k: p.graph_nodes() for k, p in plans.items()},
               us={k: statistics.median(v) for k, v in times.items()}, spread={k: [min(v), max(v)] for k, v in times.items()})
    if not plain_only:
        ms, _ = plans["obstacle_record"].record().obstacles()
        assert (ms["compared"] == (replans + 3) * n).all()
        out["obstacle_record_us"] = out["us"]["obstacle_record"] - out["us"]["plain"]
    for p in plans.values():
        p.close()
    wmap.close()
    sol.close()
    return out


def whole_flights(api, torch, g, missions, repeats, max_replans):
    import closed_loop

    n = len(g["starts"])
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    probe = api.Grid(wmap, 0.5, float(g["radius"]), float(g["z_2d"]))
    off, starts, goals = closed_loop.seeded_missions(g, probe.download(), probe.grid_min, missions, 0)
    probe.close()
    N = int(off[-1])
    models = api.obstacle_models(obstacle_specs(float(g["z_2d"])))
    device, host = _plan(api, sol, wmap, g, N, n - 1 + N_DYN, off), _plan(api, sol, wmap, g, N, n - 1 + N_DYN, off)
    for p in (device, host):
        p.set_obstacles(models)
        p.set_record(0.1)
    device.set_obstacle_record()
    device.reset(starts, goals)
    needed = device.run(max_replans, check_every=1)  # (also the warm-up of every kernel)
    host.reset(starts, goals)
    for _ in range(3):
        host.step(graph=True)
    torch.cuda.synchronize()
    times = {"run_with_obstacle_record": [], "stepped_loop": []}
    figures = {}
    for rep in range(repeats):
        order = list(times)
        for name in (order if rep % 2 == 0 else order[::-1]):
            p = device if name == "run_with_obstacle_record" else host
            p.reset(starts, goals)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "run_with_obstacle_record":
                p.run(max_replans, check_every=16)
                figures[name] = p.record().obstacles()[0]["safety_ratio_obs"].copy()
            else:
                least = np.full(missions, np.inf)
                for _ in range(needed):
                    flying = p.record().download()[0]["finished"] == 0  # (a finished mission's figure is frozen)
                    p.step(graph=True)
                    torch.cuda.synchronize()
                    v = p.get_obstacles(api.PLAN_OBS_SAFETY)["safety_ratio_obs"]
                    for k in np.flatnonzero(flying):
                        least[k] = min(least[k], float(v[int(off[k]):int(off[k + 1])].min()))
                figures[name] = least
            times[name].append((time.perf_counter() - t0) * 1e3)
    same = figures["run_with_obstacle_record"].tobytes() == figures["stepped_loop"].tobytes()
    assert same, (figures["run_with_obstacle_record"], figures["stepped_loop"])
    rec, _ = device.record().download()
    out = dict(missions=missions, agents=N, replans_needed=needed, finished=int(rec["finished"].sum()), same_figures=bool(same),
               least_figure=float(figures["stepped_loop"].min()),
               flight_ms={k: statistics.median(v) for k, v in times.items()}, spread_ms={k: [min(v), max(v)] for k, v in times.items()})
    for p in (device, host):
        p.close()
    wmap.close()
    sol.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", default=os.path.join(ROOT, "tests", "golden", "forest10_world.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replans", type=int, default=60)
    ap.add_argument("--max", type=int, default=400)
    ap.add_argument("--plain-only", action="store_true", help="time the plan without the option alone; nothing of the obstacle record is called")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    assert torch.cuda.is_available(), "obstacle_record_timing.py measures on the GPU"
    g = json.load(open(a.world))
    res = dict(library=os.path.basename(os.path.dirname(api.LIB_PATH)) + "/" + os.path.basename(api.LIB_PATH),
               one_replan=[one_replan(api, torch, g, c, a.repeats, a.replans, a.plain_only) for c in (1, 25)])
    print("(a) graph replay per replan, median of %d interleaved repeats of %d replans (%s)" % (a.repeats, a.replans, res["library"]))
    for r in res["one_replan"]:
        print("    %4d agents, %2d missions: " % (r["agents"], r["missions"])
              + ", ".join("%s %.1f us [%.1f, %.1f] (%d nodes)" % (k, r["us"][k], r["spread"][k][0], r["spread"][k][1], r["nodes"][k]) for k in r["us"])
              + ("" if a.plain_only else ", obstacle record %+.1f us" % r["obstacle_record_us"]))
    if not a.plain_only:
        w = res["whole_flights"] = whole_flights(api, torch, g, 25, a.repeats, a.max)
        print("(b) %d missions, %d agents, two obstacles, flown until every mission has finished or --max: %d replans, %d finished; least figure %.6f, the same "
              "per mission both ways: %s" % (w["missions"], w["agents"], w["replans_needed"], w["finished"], w["least_figure"], w["same_figures"]))
        for k, v in w["flight_ms"].items():
            print("    %-26s %.1f ms [%.1f, %.1f]" % (k, v, w["spread_ms"][k][0], w["spread_ms"][k][1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
