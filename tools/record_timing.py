"""What the mission record costs and what flying to the finish on the device saves (include/lscqp.h, "the mission record").

    python tools/record_timing.py [--repeats 7] [--replans 60] [--max 400] [--out FILE.json]

(a) One replan: graph replay time per replan of forest10 (one mission of 10 agents) and of 25 x forest10 (a partition of 25 missions), with
    and without a record.  Each repeat resets the plan, warms it up (the eager first replan and two replays) and times `--replans` replays
    between two device synchronisations -- the same stretch of the same flight for both plans; the two plans alternate within a repeat and
    the median over the repeats is reported.
(b) Whole flights: 25 seeded missions over the forest10 world flown to the finish -- by the host loop of tools/closed_loop.py: run_missions
    (a synchronisation and five downloads per replan, figures accumulated on the host; it cannot tell when a mission is over, so it is
    given the number of replans the device needed) and by lscqp_plan_run with check_every 1 and 16.  Wall clock around the flight, resets
    outside the window; the median over the repeats.
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


def _plan(api, sol, wmap, g, N, n_obs, off=None):
    ag = np.zeros(N, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = g["radius"], 2.0, 1.0, 2.0, 1.0
    return api.Plan(sol, wmap, N, n_obs, ag, constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True,
                    z_2d=float(g["z_2d"]), safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT, mission_offsets=off)


def one_replan(api, torch, g, copies, repeats, replans):
    n = len(g["starts"])
    starts, goals = np.tile(np.array(g["starts"], float), (copies, 1)), np.tile(np.array(g["goals"], float), (copies, 1))
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    off = np.arange(copies + 1) * n if copies > 1 else None
    plans = {"without": _plan(api, sol, wmap, g, copies * n, n - 1, off), "with": _plan(api, sol, wmap, g, copies * n, n - 1, off)}
    plans["with"].set_record(1e-3)  # (never reached within the window: the record accumulates in every replan)
    times = {k: [] for k in plans}
    for rep in range(repeats):
        for name in (("without", "with") if rep % 2 == 0 else ("with", "without")):
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
    rec = plans["with"].record().download()[0]
    assert (rec["replans"] == replans + 3).all() and not rec["finished"].any()
    same = np.array_equal(plans["with"].get(api.PLAN_PLAN), plans["without"].get(api.PLAN_PLAN))
    out = dict(agents=copies * n, missions=copies, nodes_without=plans["without"].graph_nodes(), nodes_with=plans["with"].graph_nodes(), same_plans=bool(same),
               us_without=statistics.median(times["without"]), us_with=statistics.median(times["with"]),
               spread_without=[min(times["without"]), max(times["without"])], spread_with=[min(times["with"]), max(times["with"])])
    out["record_us"] = out["us_with"] - out["us_without"]
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
    device, host = _plan(api, sol, wmap, g, N, n - 1, off), _plan(api, sol, wmap, g, N, n - 1, off)
    device.set_record(0.1)
    device.reset(starts, goals)
    needed = device.run(max_replans, check_every=1)  # (also the warm-up of every kernel)
    first = device.record().download()[0]

    def host_loop(steps):  # tools/closed_loop.py: run_missions, its loop as it stands
        per = [dict(qp_failed=0, invalid=0, min_safety_ratio=np.inf, max_vel_excess=0.0, max_acc_excess=0.0, waypoints_updated=0, truncated=0) for _ in range(missions)]
        for _ in range(steps):
            host.step(graph=True)
            torch.cuda.synchronize()
            st, valid, saf, upd, cnt = (host.get(b) for b in (api.PLAN_STATUS, api.PLAN_VALID, api.PLAN_SAFETY, api.PLAN_WAYPOINT_UPDATED, api.PLAN_IN_RANGE))
            for k, m in enumerate(per):
                sl = slice(int(off[k]), int(off[k + 1]))
                m["qp_failed"] += int((st[sl] != 0).sum())
                m["invalid"] += int(((st[sl] == 0) & (valid[sl] != 1)).sum())
                m["min_safety_ratio"] = float(min(m["min_safety_ratio"], saf["safety_ratio"][sl].min()))
                m["max_vel_excess"] = float(max(m["max_vel_excess"], saf["vel_excess_ratio"][sl].max()))
                m["max_acc_excess"] = float(max(m["max_acc_excess"], saf["acc_excess_ratio"][sl].max()))
                m["waypoints_updated"] += int(upd[sl].sum())
                m["truncated"] += int((cnt[sl] > n - 1).sum())
        return per

    host.reset(starts, goals)
    host_loop(3)
    times = {"host_loop": [], "run_every_1": [], "run_every_16": []}
    enq = {}
    for rep in range(repeats):
        order = ["host_loop", "run_every_1", "run_every_16"]
        for name in order[rep % 3:] + order[:rep % 3]:
            p = host if name == "host_loop" else device
            p.reset(starts, goals)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "host_loop":
                host_loop(needed)
            else:
                enq[name] = p.run(max_replans, check_every=1 if name == "run_every_1" else 16)
                rec = p.record().download()[0]
            times[name].append((time.perf_counter() - t0) * 1e3)
            if name != "host_loop":
                assert rec.tobytes() == first.tobytes()  # (records freeze: the same whatever check_every is)
    out = dict(missions=missions, agents=N, max_replans=max_replans, replans_needed=needed, missions_finished=int(first["finished"].sum()),
               replans_enqueued=enq, flight_ms={k: statistics.median(v) for k, v in times.items()},
               spread_ms={k: [min(v), max(v)] for k, v in times.items()},
               longest_flight_s=float(first["flight_time"].max()), total_distance_m=float(first["distance"].sum()), qp_failed=int(first["qp_failed"].sum()))
    for p in (device, host):
        p.close()
    wmap.close()
    sol.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", default=os.path.join(ROOT, "tests", "golden", "forest10_world.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--replans", type=int, default=60)
    ap.add_argument("--max", type=int, default=400)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    assert torch.cuda.is_available(), "record_timing.py measures on the GPU"
    g = json.load(open(a.world))
    res = dict(one_replan=[one_replan(api, torch, g, c, a.repeats, a.replans) for c in (1, 25)],
               whole_flights=whole_flights(api, torch, g, 25, a.repeats, a.max))
    print("(a) graph replay per replan, median of %d interleaved repeats of %d replans" % (a.repeats, a.replans))
    for r in res["one_replan"]:
        print("    %4d agents, %2d missions: without %.1f us (%d nodes), with %.1f us (%d nodes), record %+.1f us"
              % (r["agents"], r["missions"], r["us_without"], r["nodes_without"], r["us_with"], r["nodes_with"], r["record_us"]))
    w = res["whole_flights"]
    print("(b) %d missions, %d agents, %d of them finished within %d replans (needed: %d)" % (w["missions"], w["agents"], w["missions_finished"], w["max_replans"], w["replans_needed"]))
    for k, v in w["flight_ms"].items():
        print("    %-14s %.1f ms" % (k, v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
