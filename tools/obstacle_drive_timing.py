"""What the drives of chasing and gaussian obstacles cost in the replan chain (include/lscqp.h, "chasing and gaussian obstacles"), and what
they save against playing those obstacles on the host.

    python tools/obstacle_drive_timing.py plans  [--missions 1 25] [--repeats 7] [--replans 60] [--held-only] [--still]
    python tools/obstacle_drive_timing.py kernel [--launches 200] [--repeats 7]
    python tools/obstacle_drive_timing.py flight [--missions 25] [--max-replans 200] [--repeats 3]

plans   graph replay time per replan, the method of tools/obstacle_timing.py: K seeded missions over the forest10 world in one plan (10 K
        agents, M = 10, 2-D, LSC rows as tools/closed_loop.py flies obstacles by default, the device's waypoint decision) with one chaser
        after agent 0 and one gaussian obstacle, flown
        `held` (the two are plain HELD entries at their start: what the parent commit can fly) and `driven` (lscqp_plan_set_obstacle_drives);
        the two alternate within a repeat, the median over the repeats is reported with the spread.  --held-only times the held plan and
        the plan without obstacles alone: run it with LSCQP_LIB naming the parent commit's build in fresh processes, alternating with this
        build's, to compare the two builds on what both can do.  --still: the drives run in full but leave the obstacles where they are
        (gamma_target = gamma_obs = 0, no initial velocity, a history of zeros), so the driven plan flies the held plan's QPs and the
        difference is the node alone; without it the difference also holds what MOVING obstacles do to the QPs behind them.
kernel  lscqp_obstacles_drive_device + lscqp_obstacles_advance_device alone on those two obstacles, `--launches` pairs back to back between
        two events, starting at clock 1 and at clock 400 (one untimed pair first, so that the checkpoint is there): the gaussian obstacle's
        cost late in a flight against its cost at the start.  And the advance alone.
flight  K missions to the finish: lscqp_plan_run with the drives (no host work between replans) against the loop that plays the two
        obstacles on the host -- per replan one download of the state and the table, lscqp_obstacle_drive_host, one upload, one graph
        replay; the record's unfinished count read every 16 replans in both.  Host wall time of the whole flight, the two alternating.
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


def obstacle_specs(g, still=False):
    if still:
        moving = obstacle_specs(g)
        moving[0].update(gamma_target=0.0, gamma_obs=0.0)
        moving[1].update(initial_vel=[0.0, 0.0, 0.0], acc_history=np.zeros((1200, 3)))
        return moving
    z = float(g["z_2d"])
    lo, hi = np.array(g["world_min"]), np.array(g["world_max"])
    history = np.c_[np.random.default_rng(2).normal(0.0, 0.3, (1200, 2)), np.zeros(1200)]  # 120 s, in the mission's plane
    return [dict(type="chasing", start=[hi[0] - 0.2, hi[1] - 0.2, z], size=0.1, max_vel=0.3, max_acc=1.0, gamma_target=1.0, gamma_obs=1.0, downwash=1.0,
                 target_agent=0),
            dict(type="gaussian", start=[lo[0] + 0.2, lo[1] + 0.2, z], size=0.1, initial_vel=[0.05, 0.05, 0.0], max_vel=0.2, max_acc=1.0, acc_update_cycle=0.1,
                 downwash=1.0, acc_history=history)]


def mission(api, missions, seed=0, still=False):
    """(make a plan with `n_dyn` obstacle slots, starts, goals, what to close) for K seeded missions over forest10 (tools/closed_loop.py)."""
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

    def plan(n_dyn):
        return api.Plan(sol, wmap, N, n - 1 + n_dyn, ag, constraint_mode=api.GEN_LSC if n_dyn else api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True, closed_loop=True,
                        z_2d=float(g["z_2d"]), safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT,
                        mission_offsets=off if missions > 1 else None)

    return plan, obstacle_specs(g, still), starts, goals, N, (sol, wmap)


def plans(api, torch, missions, repeats, replans, held_only, still):
    plan, specs, starts, goals, N, keep = mission(api, missions, still=still)
    models = api.obstacle_models(specs)
    flown = {"held": plan(2)}
    flown["held"].set_obstacles(models)
    if held_only:
        flown["bare"] = plan(0)
    else:
        flown["driven"] = plan(2)
        flown["driven"].set_obstacles(models)
        flown["driven"].set_obstacle_drives(*api.obstacle_drives(specs, N))
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
    out = dict(missions=missions, agents=N, replans=replans, repeats=repeats, still=bool(still))
    for name, p in flown.items():
        out["qp_failed_" + name] = int((p.get(api.PLAN_STATUS) != 0).sum())
        out["us_" + name] = statistics.median(times[name])
        out["spread_" + name] = [min(times[name]), max(times[name])]
        out["nodes_" + name] = p.graph_nodes()
    if not held_only:
        out["drive_us"] = out["us_driven"] - out["us_held"]
    for p in flown.values():
        p.close()
    keep[1].close()
    keep[0].close()
    return out


def kernel(api, torch, launches, repeats):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
    specs = obstacle_specs(g)
    models = api.obstacle_model_prepare(api.obstacle_models(specs))
    drives, history = api.obstacle_drives(specs, 1)
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2, world_min=g["world_min"], world_max=g["world_max"]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    table = np.zeros(2, api.OBSTACLE_DTYPE)
    table["position"], table["radius"], table["downwash"], table["max_acc"] = np.float32(models["start"]), models["radius"], models["downwash"], models["max_acc"]
    state = np.zeros((1, 9))
    state[0, :3] = (1.0, 1.0, float(g["z_2d"]))
    d_models, d_drives, d_hist, d_state = up(models), up(drives), up(history), up(state)
    d_clock = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = dict(launches=launches, repeats=repeats)
    for what in ("drive_and_advance", "advance"):
        for clock in (1, 400):
            took = []
            for _ in range(repeats):
                d_table, d_ckpt = up(table), torch.zeros(2 * api.OBSTACLE_DRIVE_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
                d_clock.fill_(clock)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for i in range(launches + 1):
                    if i == 1:
                        e0.record()
                    if what == "drive_and_advance":
                        sol.obstacles_drive_device(d_models, d_drives, 2, d_hist, len(history), d_state, 1, d_ckpt, 0.2, d_clock, d_table)
                    sol.obstacles_advance_device(d_models, 2, 0.2, d_clock, d_table)
                e1.record()
                torch.cuda.synchronize()
                took.append(e0.elapsed_time(e1) * 1e3 / launches)
            out["%s_us_from_clock_%d" % (what, clock)] = statistics.median(took)
            out["%s_spread_from_clock_%d" % (what, clock)] = [min(took), max(took)]
    sol.close()
    return out


def flight(api, torch, missions, max_replans, repeats, check_every=16):
    plan, specs, starts, goals, N, keep = mission(api, missions)
    raw = api.obstacle_models(specs)
    models = api.obstacle_model_prepare(raw)
    drives, history = api.obstacle_drives(specs, N)
    device, host = plan(2), plan(2)
    for p in (device, host):
        p.set_obstacles(raw)
        p.set_record(0.1)
    device.set_obstacle_drives(drives, history)
    times, replans = {"device": [], "host": []}, {}
    for rep in range(repeats + 1):  # (the first repeat warms both up and is not counted)
        for name in (("device", "host") if rep % 2 == 0 else ("host", "device")):
            p = device if name == "device" else host
            p.reset(starts, goals)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "device":
                done = p.run(max_replans, check_every=check_every)
            else:
                ckpt, done = np.zeros(2, api.OBSTACLE_DRIVE_STATE_DTYPE), 0
                while done < max_replans:
                    table = p.get_obstacles()
                    keep[0].obstacle_drive_host(models, drives, history, p.get(api.PLAN_STATE), ckpt, 0.2, done, table)
                    p.put_obstacles(table)
                    p.step(graph=True)
                    done += 1
                    if done % check_every == 0 and p.record().unfinished() == 0:
                        break
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
            replans[name] = done
            replans[name + "_finished"] = int(p.record().download()[0]["finished"].sum())
    same = device.get_obstacles().tobytes() == host.get_obstacles().tobytes() and device.get(api.PLAN_PLAN).tobytes() == host.get(api.PLAN_PLAN).tobytes()
    out = dict(missions=missions, agents=N, max_replans=max_replans, repeats=repeats, replans=replans, same_final_table_and_plans=bool(same))
    for name in times:
        out["s_" + name] = statistics.median(times[name])
        out["spread_" + name] = [min(times[name]), max(times[name])]
        out["us_per_replan_" + name] = out["s_" + name] / replans[name] * 1e6
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
    ap.add_argument("--max-replans", type=int, default=200)
    ap.add_argument("--held-only", action="store_true")
    ap.add_argument("--still", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from lsc_dr_planner_amd import api

    if not torch.cuda.is_available():
        sys.exit("tools/obstacle_drive_timing.py needs a GPU")
    if a.what == "plans":
        res = dict(library=os.path.basename(api.LIB_PATH), plans=[plans(api, torch, k, a.repeats or 7, a.replans, a.held_only, a.still) for k in (a.missions or [1, 25])])
    elif a.what == "kernel":
        res = kernel(api, torch, a.launches, a.repeats or 7)
    else:
        res = flight(api, torch, (a.missions or [25])[0], a.max_replans, a.repeats or 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
