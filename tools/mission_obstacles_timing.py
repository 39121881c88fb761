"""What a replan costs with each mission's own obstacles (include/lscqp.h, "a mission's own obstacles"), and that a plan which does not use
them costs what it did.

    python tools/mission_obstacles_timing.py [--repeats 5] [--replans 60] [--shared-only] [--out FILE.json]

Graph replay time per replan of forest10 (one mission of 10 agents) and of 25 x forest10 (a partition of 25 missions), CLSC rows, n - 1 agent
slots and two obstacle slots per agent in every plan:
    none     no obstacles
    shared   two obstacles (a straight one and a patrol) in one table for all missions (lscqp_plan_set_obstacles)
    own_same 25 missions only: two obstacles of its own per mission, 50 in all (lscqp_plan_set_mission_obstacles), every mission's pair a copy of
             the shared one -- the same slots, the same number of graph nodes and the same 25 flights as `shared`: the like-for-like comparison
    own      the same with every mission's pair moved by 5 cm per mission: 25 different flights
    singles  25 missions only: 25 plans of one mission with two obstacles each, stepped in turn (one graph replay each per replan)
As tools/obstacle_record_timing.py measures: each repeat resets the plan, warms it up (the eager first replan and two replays) and times
`--replans` replays between two device synchronisations; the plans alternate within a repeat; the median over the repeats and the spread
are reported; behind the timing every plan flies the window once more, untimed, and counts the QPs that were not OPTIMAL at the first
attempt's end (a replan with such a QP also runs the solve's second pass and its rescue pass in earnest).  --shared-only times `none` and
`shared` alone and calls nothing new, so that LSCQP_LIB may name a library that predates the feature (an A/B against the parent commit, in
fresh processes).  Prints a table and one JSON line; needs a GPU."""
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

N_SLOT = 2


def obstacle_specs(z, k=0):
    """Mission k's pair: tools/obstacle_record_timing.py's straight obstacle and patrol, moved a little per mission."""
    d = 0.05 * k
    return [dict(type="straight", start=[2.0, -1.0 + d, z], goal=[-2.0, 1.0 - d, z], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0),
            dict(type="patrol", waypoints=[[-2.5, -1.5 + d, z], [2.5, -1.5 + d, z]], size=0.15, speed=0.3, max_acc=1.0, downwash=1.0)]


class Group:
    """One timed thing: a plan, or several stepped in turn."""

    def __init__(self, plans, starts, goals):
        self.plans, self.starts, self.goals = plans, starts, goals

    def reset(self):
        for p in self.plans:
            p.reset(self.starts, self.goals)

    def step(self):
        for p in self.plans:
            p.step(graph=True)

    def nodes(self):
        return self.plans[0].graph_nodes()

    def close(self):
        for p in self.plans:
            p.close()


def measure(api, torch, g, copies, repeats, replans, shared_only):
    n = len(g["starts"])
    z = float(g["z_2d"])
    one_s, one_g = np.array(g["starts"], float), np.array(g["goals"], float)
    starts, goals = np.tile(one_s, (copies, 1)), np.tile(one_g, (copies, 1))
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    off = np.arange(copies + 1) * n if copies > 1 else None

    def plan():
        return _plan(api, sol, wmap, g, copies * n, n - 1 + N_SLOT, off)

    groups = {"none": Group([plan()], starts, goals), "shared": Group([plan()], starts, goals)}
    groups["shared"].plans[0].set_obstacles(api.obstacle_models(obstacle_specs(z)))
    if copies > 1 and not shared_only:
        for name, moved in (("own_same", 0), ("own", 1)):
            groups[name] = Group([plan()], starts, goals)
            groups[name].plans[0].set_mission_obstacles([api.obstacle_models(obstacle_specs(z, k * moved)) for k in range(copies)])
        singles = [_plan(api, sol, wmap, g, n, n - 1 + N_SLOT) for _ in range(copies)]
        for k, p in enumerate(singles):
            p.set_obstacles(api.obstacle_models(obstacle_specs(z, k)))
        groups["singles"] = Group(singles, one_s, one_g)
    names = tuple(groups)
    times = {k: [] for k in names}
    for rep in range(repeats):
        for name in (names if rep % 2 == 0 else names[::-1]):
            q = groups[name]
            q.reset()
            for _ in range(3):
                q.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(replans):
                q.step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / replans * 1e6)
    failed = {}
    for name, q in groups.items():  # (untimed) the QPs of the same window that did not end OPTIMAL, and the replans that had one
        q.reset()
        bad = []
        for _ in range(replans + 3):
            q.step()
            torch.cuda.synchronize()
            bad.append(sum(int((p.get(api.PLAN_STATUS) != 0).sum()) for p in q.plans))
        failed[name] = [sum(bad), sum(1 for b in bad if b)]
    out = dict(agents=copies * n, missions=copies, nodes={k: q.nodes() for k, q in groups.items()}, not_optimal=failed,
               us={k: statistics.median(v) for k, v in times.items()}, spread={k: [min(v), max(v)] for k, v in times.items()})
    if "own" in groups:
        p = groups["own"].plans[0]
        assert p.get_obstacles(api.PLAN_OBS_CLOCK).tolist() == [replans + 3] * copies and len(p.get_obstacles()) == N_SLOT * copies
        assert out["nodes"]["own"] == out["nodes"]["own_same"] == out["nodes"]["shared"]
    for q in groups.values():
        q.close()
    wmap.close()
    sol.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", default=os.path.join(ROOT, "tests", "golden", "forest10_world.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replans", type=int, default=60)
    ap.add_argument("--shared-only", action="store_true", help="time the plans without and with a shared table alone; nothing of the feature is called")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    assert torch.cuda.is_available(), "mission_obstacles_timing.py measures on the GPU"
    g = json.load(open(a.world))
    res = dict(library=os.path.basename(os.path.dirname(api.LIB_PATH)) + "/" + os.path.basename(api.LIB_PATH),
               one_replan=[measure(api, torch, g, c, a.repeats, a.replans, a.shared_only) for c in (1, 25)])
    print("graph replay per replan, median of %d interleaved repeats of %d replans (%s)" % (a.repeats, a.replans, res["library"]))
    for r in res["one_replan"]:
        print("    %4d agents, %2d missions: " % (r["agents"], r["missions"])
              + ", ".join("%s %.1f us [%.1f, %.1f] (%d nodes; %d QPs not OPTIMAL in %d replans)"
                          % (k, r["us"][k], r["spread"][k][0], r["spread"][k][1], r["nodes"][k], r["not_optimal"][k][0], r["not_optimal"][k][1]) for k in r["us"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
