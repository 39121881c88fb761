"""What the flight log costs per replan and what it saves over a whole flight (include/lscqp.h, "the flight log").

    python tools/flight_log_timing.py [--repeats 5] [--replans 60] [--max 400] [--capacity 400] [--record-only] [--out FILE.json]

(a) One replan: graph replay time per replan of forest10 (one mission of 10 agents) and of 25 x forest10 (a partition of 25 missions) with a
    record, and with a record and a flight log of `--capacity` rows.  As tools/record_timing.py measures the record: each repeat resets the
    plan, warms it up (the eager first replan and two replays) and times `--replans` replays between two device synchronisations; the two
    plans alternate within a repeat; the median over the repeats and the spread are reported.  --record-only times the plan with a record
    alone and calls nothing of the log, so that LSCQP_LIB may name a library that predates it (an A/B against the parent commit, in fresh
    processes).
(b) Whole flights: 25 seeded missions over the forest10 world flown to the finish by lscqp_plan_run (check_every 16) with a log, every
    mission's log downloaded behind the flight -- against the two host loops that are the other way to the same states: one eager step, or one
    graph replay, then a synchronisation and a download of LSCQP_PLAN_BUF_PLAN per replan, for the number of replans the device needed.
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


def one_replan(api, torch, g, copies, repeats, replans, capacity, record_only):
    n = len(g["starts"])
    starts, goals = np.tile(np.array(g["starts"], float), (copies, 1)), np.tile(np.array(g["goals"], float), (copies, 1))
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    off = np.arange(copies + 1) * n if copies > 1 else None
    names = ("record",) if record_only else ("record", "log")
    plans = {k: _plan(api, sol, wmap, g, copies * n, n - 1, off) for k in names}
    for k, p in plans.items():
        p.set_record(1e-3)  # (never reached within the window: record and log work in every replan)
        if k == "log":
            p.set_flight_log(capacity)
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
    if not record_only:
        assert plans["log"].record().log_rows()[0].tolist() == [min(replans + 3, capacity)] * copies
        out["log_us"] = out["us"]["log"] - out["us"]["record"]
    for p in plans.values():
        p.close()
    wmap.close()
    sol.close()
    return out


def whole_flights(api, torch, g, missions, repeats, max_replans, capacity):
    import closed_loop

    n = len(g["starts"])
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    probe = api.Grid(wmap, 0.5, float(g["radius"]), float(g["z_2d"]))
    off, starts, goals = closed_loop.seeded_missions(g, probe.download(), probe.grid_min, missions, 0)
    probe.close()
    N = int(off[-1])
    device, host = _plan(api, sol, wmap, g, N, n - 1, off), _plan(api, sol, wmap, g, N, n - 1, off)
    device.set_record(0.1)
    device.set_flight_log(capacity)
    device.reset(starts, goals)
    needed = device.run(max_replans, check_every=1)  # (also the warm-up of every kernel)
    rows = device.record().log_rows()[0]
    host.reset(starts, goals)
    for graph in (False, True, True):
        host.step(graph=graph)
    torch.cuda.synchronize()
    times = {"run_with_log": [], "host_loop_eager": [], "host_loop_graph": []}
    for rep in range(repeats):
        order = list(times)
        for name in order[rep % 3:] + order[:rep % 3]:
            p = device if name == "run_with_log" else host
            p.reset(starts, goals)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "run_with_log":
                p.run(max_replans, check_every=16)
                logs = [p.record().log(k) for k in range(missions)]
            else:
                for _ in range(needed):
                    p.step(graph=(name == "host_loop_graph"))
                    torch.cuda.synchronize()
                    p.get(api.PLAN_PLAN)
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = dict(missions=missions, agents=N, replans_needed=needed, rows=[int(r) for r in rows], log_bytes=int(sum(a.nbytes for lg in logs for a in lg)),
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
    ap.add_argument("--capacity", type=int, default=400)
    ap.add_argument("--record-only", action="store_true", help="time the plan with a record alone; nothing of the log is called")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    assert torch.cuda.is_available(), "flight_log_timing.py measures on the GPU"
    g = json.load(open(a.world))
    res = dict(library=os.path.basename(os.path.dirname(api.LIB_PATH)) + "/" + os.path.basename(api.LIB_PATH),
               one_replan=[one_replan(api, torch, g, c, a.repeats, a.replans, a.capacity, a.record_only) for c in (1, 25)])
    print("(a) graph replay per replan, median of %d interleaved repeats of %d replans (%s)" % (a.repeats, a.replans, res["library"]))
    for r in res["one_replan"]:
        print("    %4d agents, %2d missions: " % (r["agents"], r["missions"])
              + ", ".join("%s %.1f us [%.1f, %.1f] (%d nodes)" % (k, r["us"][k], r["spread"][k][0], r["spread"][k][1], r["nodes"][k]) for k in r["us"])
              + ("" if a.record_only else ", log %+.1f us" % r["log_us"]))
    if not a.record_only:
        w = res["whole_flights"] = whole_flights(api, torch, g, 25, a.repeats, a.max, a.capacity)
        print("(b) %d missions, %d agents, flown until every mission has finished or --max: %d replans; the logs: %d bytes" % (w["missions"], w["agents"], w["replans_needed"], w["log_bytes"]))
        for k, v in w["flight_ms"].items():
            print("    %-16s %.1f ms [%.1f, %.1f]" % (k, v, w["spread_ms"][k][0], w["spread_ms"][k][1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
