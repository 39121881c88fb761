"""What patrol missions cost in the replan chain (include/lscqp.h, "patrol missions"), and what they save against turning agents on the host.

    python tools/patrol_timing.py plans  [--missions 1 25] [--repeats 7] [--replans 60] [--bare-only]
    python tools/patrol_timing.py kernel [--launches 200] [--repeats 7]
    python tools/patrol_timing.py flight [--missions 25] [--max-replans 400] [--repeats 3]

plans   graph replay time per replan, the method of tools/obstacle_drive_timing.py: K seeded missions over the forest10 world in one plan (10 K
        agents, M = 10, 2-D, the device's waypoint decision), flown `bare` (no patrol: what the parent commit flies) and `patrol` with threshold
        0 -- both nodes run in full and nobody turns, the common case, so the two plans fly the same QPs and the difference is the two nodes;
        the two alternate within a repeat, the median over the repeats is reported with the spread.  --bare-only times the bare plan alone:
        run it with LSCQP_LIB naming the parent commit's build in fresh processes, alternating with this build's.
kernel  lscqp_patrol_device + lscqp_field_exchange_device alone, `--launches` pairs back to back between two events, for 10 and 250 agents
        over forest10's 441 nodes: with a threshold of 0 (nobody turns) and with one so large that EVERY agent turns in every call, the
        exchange's worst case.
flight  K missions for max_replans replans: lscqp_plan_run with the patrol (no host work between replans) against the only way the parent
        commit offers -- per replan one graph replay and one download of the states, arrivals tested on the host, and at every arrival an
        lscqp_plan_reset from the agents' positions with the turned agents' goals exchanged.  That reset puts every agent of the plan at
        rest and throws away the plans, corridors, record and flight log, so the two do NOT fly the same flight: the legs completed by
        each are reported beside the host wall time.
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


def mission(api, missions, seed=0):
    from tools import closed_loop as CL

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
    n = len(g["starts"])
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    off = np.arange(missions + 1) * n
    if missions > 1:
        probe = api.Grid(wmap, 0.5, float(g["radius"]), float(g["z_2d"]))
        _, starts, goals = CL.seeded_missions(g, probe.download(), probe.grid_min, missions, seed)
        probe.close()
    else:
        starts, goals = np.array(g["starts"], float), np.array(g["goals"], float)
    N = int(off[-1])
    ag = np.zeros(N, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = g["radius"], 2.0, 1.0, 2.0, 1.0

    def plan():
        return api.Plan(sol, wmap, N, n - 1, ag, constraint_mode=api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True,
                        z_2d=float(g["z_2d"]), safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT,
                        mission_offsets=off if missions > 1 else None)

    return plan, starts, goals, N, float(g["z_2d"]), (sol, wmap)


def plans(api, torch, missions, repeats, replans, bare_only):
    plan, starts, goals, N, _, keep = mission(api, missions)
    flown = {"bare": plan()}
    if not bare_only:
        flown["patrol"] = plan()
        flown["patrol"].set_patrol(0.0)
    times, names = {k: [] for k in flown}, list(flown)
    for rep in range(repeats):
        for name in (names if rep % 2 == 0 else names[::-1]):
            p = flown[name]
            p.reset(starts, goals)
            for _ in range(3):
                p.step(graph=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(replans):
                p.step(graph=True)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / replans * 1e6)
    out = dict(missions=missions, agents=N, replans=replans, repeats=repeats)
    for name, p in flown.items():
        out["qp_failed_" + name] = int((p.get(api.PLAN_STATUS) != 0).sum())
        out["us_" + name] = statistics.median(times[name])
        out["spread_" + name] = [min(times[name]), max(times[name])]
        out["nodes_" + name] = p.graph_nodes()
    if not bare_only:
        out["two_nodes_us"] = out["us_patrol"] - out["us_bare"]
        out["same_plans"] = flown["bare"].get(api.PLAN_PLAN).tobytes() == flown["patrol"].get(api.PLAN_PLAN).tobytes()
    for p in flown.values():
        p.close()
    keep[1].close()
    keep[0].close()
    return out


def kernel(api, torch, launches, repeats, nodes=441):
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2))
    out = dict(launches=launches, repeats=repeats, nodes=nodes)
    for n in (10, 250):
        rnd = np.random.default_rng(n)
        state = torch.from_numpy(rnd.uniform(-4, 4, (n, 9))).cuda()
        for name, thr in (("nobody_turns", 0.0), ("everybody_turns", 1e6)):
            took = []
            for _ in range(repeats):
                d, s = torch.from_numpy(rnd.uniform(-4, 4, (n, 3))).cuda(), torch.from_numpy(rnd.uniform(-4, 4, (n, 3))).cuda()
                legs, sw = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
                f, o = torch.zeros(n * nodes, dtype=torch.int32, device="cuda"), torch.ones(n * nodes, dtype=torch.int32, device="cuda")
                di, do = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for i in range(launches + 1):
                    if i == 1:
                        e0.record()
                    sol.patrol_device(n, state, d, s, thr, 2, 0.6, legs, sw)
                    sol.field_exchange_device(n, nodes, sw, f, o, di, do)
                e1.record()
                torch.cuda.synchronize()
                assert int(legs.sum()) == (0 if thr == 0.0 else n * (launches + 1))
                took.append(e0.elapsed_time(e1) * 1e3 / launches)
            out["pair_us_%s_%d_agents" % (name, n)] = statistics.median(took)
            out["pair_spread_%s_%d_agents" % (name, n)] = [min(took), max(took)]
    sol.close()
    return out


def flight(api, torch, missions, max_replans, repeats, threshold=0.1, check_every=16):
    plan, starts, goals, N, z, keep = mission(api, missions)
    f32 = lambda a: np.float32(a).astype(np.float64)  # noqa: E731
    device, host = plan(), plan()
    for p in (device, host):
        p.set_record(threshold)
    device.set_patrol(threshold)
    times, legs, resets = {"device": [], "host": []}, {}, 0
    for rep in range(repeats + 1):  # (the first repeat warms both up and is not counted)
        for name in (("device", "host") if rep % 2 == 0 else ("host", "device")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "device":
                device.reset(starts, goals)
                done = device.run(max_replans, check_every=check_every)
                torch.cuda.synchronize()
                took = time.perf_counter() - t0
                legs[name] = int(device.patrol(api.PATROL_LEGS).sum())
            else:
                want, back, count, resets = f32(goals), f32(starts), 0, 0
                want[:, 2] = back[:, 2] = float(np.float32(z))
                host.reset(starts, goals)
                for done in range(1, max_replans + 1):
                    host.step(graph=True)
                    pos = np.float32(host.get(api.PLAN_STATE).reshape(N, 9)[:, :3])  # (waits for the replan)
                    e = np.float32(want) - pos
                    near = np.sqrt(np.float64(np.float32(np.float32(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]))) < threshold
                    if near.any():
                        want[near], back[near] = back[near].copy(), want[near].copy()
                        count += int(near.sum())
                        resets += 1
                        host.reset(np.float64(pos), want)
                torch.cuda.synchronize()
                took = time.perf_counter() - t0
                legs[name] = count
            if rep:
                times[name].append(took)
    out = dict(missions=missions, agents=N, max_replans=max_replans, repeats=repeats, goal_threshold=threshold, legs=legs, host_resets=resets)
    for name in times:
        out["s_" + name] = statistics.median(times[name])
        out["spread_" + name] = [min(times[name]), max(times[name])]
        out["us_per_replan_" + name] = out["s_" + name] / max_replans * 1e6
    for p in (device, host):
        p.close()
    keep[1].close()
    keep[0].close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("plans", "kernel", "flight"))
    ap.add_argument("--missions", type=int, nargs="+", default=None)
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--replans", type=int, default=60)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--max-replans", type=int, default=400)
    ap.add_argument("--bare-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    if not torch.cuda.is_available():
        sys.exit("tools/patrol_timing.py needs a GPU")
    if a.what == "plans":
        res = dict(library=os.path.basename(os.path.dirname(api.LIB_PATH)) + "/" + os.path.basename(api.LIB_PATH),
                   plans=[plans(api, torch, k, a.repeats or 7, a.replans, a.bare_only) for k in (a.missions or [1, 25])])
    elif a.what == "kernel":
        res = kernel(api, torch, a.launches, a.repeats or 7)
    else:
        res = flight(api, torch, (a.missions or [25])[0], a.max_replans, a.repeats or 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "a").write(line + "\n")
