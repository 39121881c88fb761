"""Closed-loop replanning with every row of the path on the device, in the reference's default configuration
(mode/planner = lsc, mode/goal = grid_based_planner: generateCLSC + constructSFCFromConvexHull + GoalOptimizer + TrajOptimizer):

    world boxes -> voxel map -> [ per replan: shift previous plans -> neighbours in range -> corridors -> CLSC rows -> goal LP -> trajectory QP
                                  -> isSolValid / next state -> safety metrics ]

    python tools/closed_loop.py [--steps 40] [--world tests/golden/forest10_world.json]
    python tools/closed_loop.py --missions 25 --until-finished [MAX]      (K seeded missions in one plan, flown to the finish on the device)
    python tools/closed_loop.py --missions 4 --worlds A.csv B.csv C.csv D.csv   (mission k over world k: one plan, a world per mission)
    python tools/closed_loop.py --missions 3 --obstacles A.json B.json C.json [--drive-obstacles] [--until-finished]   (mission k among file k's obstacles)
    python tools/closed_loop.py --patrol [--goal-threshold T] [--missions K] --steps 400   (a patrol: legs per agent, per mission)

The host keeps the per-agent headers and, with --router host (the default), picks each agent's next waypoint with a stand-in
for the grid-based planner (8-connected shortest paths, no conflict handling between agents).  --router device replaces
the stand-in by lscqp_waypoints_device: the reference's own rule (4-connected grid, one PIBT step per communication
group, the simulator's update filter), so its paths differ from the stand-in's.  Agents whose QP fails or whose solution is invalid keep their shifted previous plan, like the reference
(src/traj_planner.cpp:767-797).  Prints one JSON summary; tests/test_closed_loop.py runs it.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class GridRouter:
    """Stand-in for the reference's grid-based planner (out of scope: src/grid_based_planner.cpp, MAPF): shortest paths on
    the 0.5 m grid of launch/simulation.launch:88 around the inflated obstacles, one agent at a time (no conflict
    resolution between agents -- the LSCs keep them apart)."""

    def __init__(self, g, occ, key0, spacing=0.5):
        self.sp, self.wmin, self.wmax = spacing, np.array(g["world_min"][:2]), np.array(g["world_max"][:2])
        self.n = np.round((self.wmax - self.wmin) / spacing).astype(int) + 1
        res, reach = g["resolution"], g["radius"] + 0.1
        zk = int(np.floor(g["z_2d"] / res)) - key0[2]
        plane = occ[zk]
        self.free = np.zeros(self.n, bool)
        for i in range(self.n[0]):
            for j in range(self.n[1]):
                p = self.wmin + spacing * np.array([i, j])
                a = np.floor((p - reach) / res + 1e-6).astype(int) - key0[:2]
                b = np.ceil((p + reach) / res - 1e-6).astype(int) - key0[:2]
                a, b = np.maximum(a, 0), np.minimum(b, [plane.shape[1], plane.shape[0]])
                self.free[i, j] = not plane[a[1]:b[1], a[0]:b[0]].any()
        self.dist = {}

    def node(self, p):
        return tuple(np.clip(np.round((np.asarray(p[:2]) - self.wmin) / self.sp).astype(int), 0, self.n - 1))

    def field(self, goal):  # BFS distance-to-goal over free nodes (8-connected, no corner cutting)
        key = self.node(goal)
        if key in self.dist:
            return self.dist[key]
        D = np.full(self.n, np.inf)
        D[key] = 0
        todo = [key]
        while todo:
            nxt = []
            for (i, j) in todo:
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        a, b = i + di, j + dj
                        if (di or dj) and 0 <= a < self.n[0] and 0 <= b < self.n[1] and self.free[a, b]:
                            if di and dj and not (self.free[i + di, j] and self.free[i, j + dj]):
                                continue
                            w = D[i, j] + (1.4142 if di and dj else 1.0)
                            if w < D[a, b] - 1e-9:
                                D[a, b] = w
                                nxt.append((a, b))
            todo = nxt
        self.dist[key] = D
        return D

    def next_waypoint(self, pos, goal):
        D = self.field(goal)
        i, j = self.node(pos)
        best, arg = D[i, j], (i, j)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                a, b = i + di, j + dj
                if 0 <= a < self.n[0] and 0 <= b < self.n[1] and self.free[a, b] and D[a, b] < best - 1e-9:
                    if di and dj and not (self.free[i + di, j] and self.free[i, j + dj]):
                        continue
                    best, arg = D[a, b], (a, b)
        return self.wmin + self.sp * np.array(arg), self.wmin + self.sp * np.array([i, j])


def random_forest_world(n_agents=64, side=24.0, n_boxes=150, seed=0, clearance=0.8):
    """A synthetic 2-D forest in the reference's world format (pillars 0.5 x 0.5 x 2.5 m, like world/forest/*.csv) with
    n_agents start / goal pairs on opposite sides of a circle (the antipodal swap of the reference's missions), all on the
    0.5 m grid and clear of the pillars."""
    rng = np.random.default_rng(seed)
    half = side / 2
    ang = np.linspace(0, 2 * np.pi, n_agents, endpoint=False)
    starts = np.round(np.c_[np.cos(ang), np.sin(ang)] * (half - 2.0) / 0.5) * 0.5
    goals = -starts
    boxes = []
    while len(boxes) < n_boxes:
        c = rng.uniform(-half + 1, half - 1, 2)
        if np.abs(starts - c).max(axis=1).min() < clearance or np.abs(goals - c).max(axis=1).min() < clearance:
            continue
        boxes.append([c[0], c[1], 1.25, 0.5, 0.5, 2.5])
    z = 0.6
    return {"boxes": boxes, "world_min": [-half, -half, 0.0], "world_max": [half, half, 2.5], "resolution": 0.1, "max_dist": 1.0,
            "z_2d": z, "radius": 0.15, "starts": [[p[0], p[1], z] for p in starts], "goals": [[p[0], p[1], z] for p in goals]}


def seeded_mission(world, occ, grid_min, k, seed=0):
    """Mission k over the grid occupancy `occ`: mission 0 is the world's own, mission k > 0 has as many agents on distinct free grid nodes and
    distinct free goal nodes drawn from (seed, k).  Returns (starts, goals)."""
    if k == 0:
        return np.array(world["starts"], float), np.array(world["goals"], float)
    n = len(world["starts"])
    ys, xs = np.nonzero(~occ.astype(bool))
    pick = np.random.default_rng([seed, k]).choice(len(xs), size=2 * n, replace=False)
    pts = np.c_[grid_min[0] + 0.5 * xs[pick], grid_min[1] + 0.5 * ys[pick], np.full(2 * n, float(world["z_2d"]))]
    return pts[:n], pts[n:]


def seeded_missions(world, occ, grid_min, missions, seed=0):
    """K missions over one world (seeded_mission for k = 0 .. K - 1).  Returns (offsets [K + 1], starts, goals)."""
    per = [seeded_mission(world, occ, grid_min, k, seed) for k in range(missions)]
    return np.arange(missions + 1) * len(world["starts"]), np.concatenate([m[0] for m in per]), np.concatenate([m[1] for m in per])


def load_worlds(spec, missions):
    """Box lists ((n, 6) arrays: centre xyz, size xyz), one per mission, for `worlds=`: a directory of world CSVs (its *.csv in natural order,
    as Mission::loadMission lists a world directory), a list of CSV paths, or a list of box lists.  Exactly `missions` of them: the
    reference pairs mission k with world k only when the two lists are equally long.  No device needed."""
    if isinstance(spec, (str, os.PathLike)):
        spec = [spec]
    spec = list(spec)
    if len(spec) == 1 and isinstance(spec[0], (str, os.PathLike)) and os.path.isdir(spec[0]):
        d = os.fspath(spec[0])
        names = sorted((f for f in os.listdir(d) if f.endswith(".csv")), key=lambda f: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", f)])
        spec = [os.path.join(d, f) for f in names]
    if not missions or len(spec) != int(missions):
        raise ValueError("worlds: %d worlds for missions=%s -- one world per mission required" % (len(spec), missions))
    out = []
    for w in spec:
        if isinstance(w, (str, os.PathLike)):
            if not os.path.isfile(w):
                raise ValueError("worlds: no such world file: %s" % os.fspath(w))
            rows = [line.replace(",", " ").split() for line in open(w)]
            w = [[float(v) for v in r[:6]] for r in rows if len(r) >= 6]
        b = np.asarray(w, dtype=np.float64).reshape(-1, 6)
        out.append(b)
    return out


def load_obstacles(path):
    """The reference's mission-file obstacle list (missions/*.json: "obstacles": [{"type", "start", "goal", "waypoints", "axis", "size", "speed",
    "max_acc", "downwash"}, ...]; a bare list is taken too) as api.OBSTACLE_MODEL_DTYPE records.  2-D worlds: the file gives z as well."""
    from lsc_dr_planner_amd import api

    return api.obstacle_models(load_obstacle_specs(path))


def load_obstacle_specs(path):
    """The same list as it stands in the file: what api.obstacle_drives reads the chasing and gaussian entries' parameters from."""
    doc = json.load(open(path))
    return doc["obstacles"] if isinstance(doc, dict) else doc


def _g(v):
    """A number as std::ostream prints it by default, which is how the reference writes its logs: printf's %g, six significant digits."""
    return "%g" % float(v)


def write_flight_csv(path, states, obstacles, time_step, record_time_step, planning_time=0.0):
    """One mission's flight log (api.Record.log: states (rows, n, S, 9), obstacles (rows, n_dyn, 4)) as the reference's result log
    (MultiSyncSimulator::saveSimulationResultAsCSV, src/multi_sync_simulator.cpp:586-656; the shim's SimulationResultCsv::writeFlight writes
    the same file): per agent "id,t,px,py,pz,vx,vy,vz,ax,ay,az,planning_time", per obstacle "obs_id,t,px,py,pz,size", one line per sample
    time.  planning_time is host wall time, which the device log does not hold: the caller's, one number or (rows, n) per replan and agent."""
    rows, n, S, _ = states.shape
    n_dyn = obstacles.shape[1]
    pt = np.broadcast_to(np.asarray(planning_time, np.float64), (rows, n))
    with open(path, "w") as f:
        f.write(",".join(["id,t,px,py,pz,vx,vy,vz,ax,ay,az,planning_time"] * n + ["obs_id,t,px,py,pz,size"] * n_dyn) + "\n")
        for r in range(rows):
            for s in range(S):
                t = _g(r * time_step + s * record_time_step)
                fields = []
                for q in range(n):
                    fields += [str(q), t] + [_g(v) for v in states[r, q, s]] + [_g(pt[r, q])]
                for o in range(n_dyn):
                    fields += [str(o), t] + [_g(v) for v in obstacles[r, o]]
                f.write(",".join(fields) + "\n")


def run_missions(world_json, missions, steps=40, M=10, dt=0.2, n_obs=None, seed=0, graph=True, until_finished=None, check_every=16,
                 goal_threshold=0.1, obstacles=None, worlds=None, obstacle_rows="lsc", log_csv=None, obstacle_specs=None, obstacle_seed=0, patrol=None,
                 mission_obstacles=None, mission_obstacle_specs=None):
    """`missions` seeded missions over one world flown by ONE lscqp_plan with a mission partition (include/lscqp.h, "many missions over one
    map"): waypoint_mode 1, closed loop, one captured graph per replan.  The summary has the figures of `run` per mission.
    until_finished = MAX: the plan keeps a mission record (include/lscqp.h, "the mission record") and lscqp_plan_run flies it until every
    mission has finished or MAX replans, with no download in between; per mission the summary then holds the device's record -- and with
    obstacles the mission's obstacle record (include/lscqp.h, "the obstacle record"): obstacle_safety_ratio, the least agent-obstacle safety
    ratio of the flight, with its replan, agent and obstacle, and below_one, the agent-replans whose figure was below 1.
    obstacles: api.OBSTACLE_MODEL_DTYPE records (load_obstacles) -- the dynamic obstacles every mission shares, moved by the chain itself
    (lscqp_plan_set_obstacles).  obstacle_rows "lsc": their rows are generateLSC's, so the agents' rows are LSC rows too (GEN_LSC instead
    of GEN_CLSC); "clsc": the plan stays in GEN_CLSC, the mode the reference's launch files run, and the obstacles get generateCLSC's rows
    like an in-range agent.  They take the first row slots: n_obs counts the agent slots, the plan gets n_obs + len(obstacles).
    obstacle_specs (with obstacles: the mission-file entries the models were made from, load_obstacle_specs): the chasing and gaussian entries
    are driven on the device (include/lscqp.h, "chasing and gaussian obstacles"; api.obstacle_drives with obstacle_seed for the gaussian
    histories, drawn for the whole flight); without it such an entry is HELD at its start.
    mission_obstacles: instead of `obstacles`, a list of `missions` arrays of such records (an empty one or None: no obstacle) -- mission k flies
    among its own and sees no other's (include/lscqp.h, "a mission's own obstacles"; lscqp_plan_set_mission_obstacles).  They take as many row
    slots as the largest list has entries.  mission_obstacle_specs: the files' entries per mission, for the drives; a chaser's target_agent is
    an agent of ITS mission, counted from that mission's first agent as the mission's own file counts it.  No flight log with them.
    worlds: one world per mission (load_worlds) in the world's box -- mission k flies over world k (include/lscqp.h, "each mission over its
    own world"; lscqp_plan_set_worlds), its seeded agents drawn from the free nodes of its own world; world 0 replaces the world's own boxes.
    log_csv (with until_finished): a directory; the plan keeps a flight log of MAX rows per mission (include/lscqp.h, "the flight log") and
    every mission's result log is written there in the reference's format, mission_<k>.csv (write_flight_csv).
    patrol = T: the plan flies a patrol (include/lscqp.h, "patrol missions"; lscqp_plan_set_patrol with goal_threshold T): every agent swaps
    start and goal on arrival, no mission finishes, and the summary holds the legs every agent completed, per mission."""
    if log_csv and not until_finished:
        raise ValueError("log_csv needs until_finished=MAX: the flight log's capacity")
    world_boxes = None if worlds is None else load_worlds(worlds, missions)  # (before anything needs a device)
    import torch

    from lsc_dr_planner_amd import api

    g = world_json if isinstance(world_json, dict) else json.load(open(world_json))
    n = len(g["starts"])
    sol = api.Solver(api.make_desc(M=M, dim=2, dt=dt, world_min=g["world_min"], world_max=g["world_max"]))
    maps = [api.WorldMap(b, g["world_min"], g["world_max"], g["resolution"], g["max_dist"]) for b in (world_boxes or [g["boxes"]])]
    wmap = maps[0]
    off = np.arange(missions + 1) * n
    probe = api.Grid(wmap, 0.5, float(g["radius"]), float(g["z_2d"]))
    if world_boxes:  # mission k's agents: (seed, k) over the free nodes of the world it flies over
        probe.set_worlds(api.Worlds(maps))
        per = [seeded_mission(g, probe.download_world(k), probe.grid_min, k, seed) for k in range(missions)]
        starts, goals = np.concatenate([m[0] for m in per]), np.concatenate([m[1] for m in per])
    else:
        _, starts, goals = seeded_missions(g, probe.download(), probe.grid_min, missions, seed)
    probe.close()
    N = int(off[-1])
    if obstacle_rows not in ("lsc", "clsc"):
        raise ValueError("obstacle_rows must be 'lsc' or 'clsc'")
    if mission_obstacles is not None:
        if obstacles is not None or len(mission_obstacles) != missions:
            raise ValueError("mission_obstacles: one list per mission (%d for missions=%d), and no shared `obstacles` beside them" % (len(mission_obstacles), missions))
        if log_csv:
            raise ValueError("log_csv: the flight log's obstacle columns are those of one shared table, not of a table per mission")
        mission_obstacles = [np.zeros(0, api.OBSTACLE_MODEL_DTYPE) if m is None else m for m in mission_obstacles]
    n_dyn = (0 if obstacles is None else len(obstacles)) if mission_obstacles is None else sum(len(m) for m in mission_obstacles)
    n_slot = n_dyn if mission_obstacles is None else max(len(m) for m in mission_obstacles)  # the row slots the obstacles take
    n_obs = max(1, min((n - 1 if n_obs is None else n_obs) + n_slot, sol.max_obstacles()))
    ag = np.zeros(N, api.AGENT_PARAM_DTYPE)
    ag["radius"], ag["downwash"], ag["max_vel"], ag["max_acc"], ag["nominal_velocity"] = g["radius"], 2.0, 1.0, 2.0, 1.0
    plan = api.Plan(sol, wmap, N, n_obs, ag, constraint_mode=api.GEN_LSC if n_dyn and obstacle_rows == "lsc" else api.GEN_CLSC, sfc_mode=api.SFC_FROM_HULL, optimize_goal=True,
                    closed_loop=True, z_2d=float(g["z_2d"]), safety_samples=2, record_time_step=0.1, waypoint_mode=api.WAYPOINT_GRID_PIBT,
                    mission_offsets=off)
    world_set = None
    if world_boxes:
        world_set = api.Worlds(maps)
        plan.set_worlds(world_set)
    if n_dyn and mission_obstacles is not None:
        plan.set_mission_obstacles(mission_obstacles)
        if mission_obstacle_specs is not None:  # one list in mission order, every chaser's target made a global agent id
            obstacle_specs = [dict(o, target_agent=int(o["target_agent"]) + int(off[k])) if int(o.get("target_agent", -1)) >= 0 else o
                              for k, per_k in enumerate(mission_obstacle_specs) for o in (per_k or [])]
    elif n_dyn:
        plan.set_obstacles(obstacles)
    n_driven = 0
    if n_dyn and obstacle_specs is not None:
        drives, history = api.obstacle_drives(obstacle_specs, N, horizon=((until_finished or steps) + 1) * dt, seed=obstacle_seed)
        plan.set_obstacle_drives(drives, history)
        n_driven = int((drives["kind"] != api.DRIVE_NONE).sum())
    if patrol is not None:
        plan.set_patrol(float(patrol))
    if until_finished:
        plan.set_record(goal_threshold)
        if log_csv:
            plan.set_flight_log(int(until_finished))
        if n_dyn:  # each mission's least obstacle safety ratio over the flight, kept beside its record (include/lscqp.h, "the obstacle record")
            plan.set_obstacle_record()
        plan.reset(starts, goals)
        enqueued = plan.run(int(until_finished), check_every=check_every, graph=graph)
        rec, _ = plan.record().download()
        csv_files = []
        if log_csv:
            os.makedirs(log_csv, exist_ok=True)
            for k in range(missions):
                st, _, ob = plan.record().log(k)
                csv_files.append(os.path.join(log_csv, "mission_%d.csv" % k))
                write_flight_csv(csv_files[-1], st, ob, dt, 0.1)
        status = plan.mission_status()
        per = [dict(mission=k, agents=n, finished=int(r["finished"]), replans=int(r["replans"]), flight_time_s=float(r["flight_time"]),
                    flight_distance_m=float(r["distance"]), qp_failed=int(r["qp_failed"]), first_qp_failed_replan=int(r["first_qp_failed_replan"]),
                    invalid=int(r["invalid"]), goal_failed=int(r["goal_failed"]), sfc_kept=int(r["sfc_kept"]), min_safety_ratio=float(r["safety_ratio_agent"]),
                    safety_replan=int(r["safety_replan"]), safety_agents=[int(r["safety_agent"]), int(r["safety_other"])],
                    max_vel_excess=float(np.linalg.norm(np.float32(r["vel_excess_ratio"]))), max_acc_excess=float(np.linalg.norm(np.float32(r["acc_excess_ratio"]))),
                    waypoints_updated=int(r["waypoint_updates"]), max_in_range=int(r["max_in_range"]), truncated_agent_steps=int(r["truncated"]),
                    walk_bound_reached=int(status[k])) for k, r in enumerate(rec)]
        if n_dyn:
            for m, o in zip(per, plan.record().obstacles()[0]):
                m.update(obstacle_safety_ratio=float(o["safety_ratio_obs"]), obstacle_safety_replan=int(o["replan"]), obstacle_safety_agent=int(o["agent"]),
                         obstacle_safety_obstacle=int(o["obstacle"]), below_one=int(o["below_one"]), safety_ratio_obs=float(o["safety_ratio_obs"]))
        if patrol is not None:
            legs = plan.patrol(api.PATROL_LEGS)
            for k, m in enumerate(per):
                m["legs"] = [int(v) for v in legs[int(off[k]):int(off[k + 1])]]
        log = dict(until_finished=int(until_finished), check_every=check_every, goal_threshold=goal_threshold, replans_enqueued=enqueued, missions=missions,
                   agents=N, row_slots=n_obs, router="device", sim_time_s=enqueued * dt, graph_nodes=plan.graph_nodes(),
                   finished=sum(m["finished"] for m in per), qp_failed=sum(m["qp_failed"] for m in per), invalid=sum(m["invalid"] for m in per),
                   min_safety_ratio=min(m["min_safety_ratio"] for m in per), per_mission=per)
        if patrol is not None:
            log.update(patrol_goal_threshold=float(patrol), legs=sum(sum(m["legs"]) for m in per))
        if n_dyn:  # (the flight's least figure per mission is in per_mission; the last replan's is what the plan still holds)
            log.update(obstacles=n_dyn, obstacle_slots=n_slot, obstacles_per_mission=mission_obstacles is not None, driven_obstacles=n_driven,
                       min_obstacle_safety_ratio=min(m["obstacle_safety_ratio"] for m in per),
                       last_obstacle_safety_ratio=float(plan.get_obstacles(api.PLAN_OBS_SAFETY)["safety_ratio_obs"].min()))
        if world_set:
            log["worlds"] = len(world_set)
        if log_csv:
            log["log_csv"] = csv_files
        plan.close()
        if world_set:
            world_set.close()
        for m_ in maps:
            m_.close()
        return log
    plan.reset(starts, goals)
    min_obstacle_ratio = np.inf
    per = [dict(mission=k, agents=n, qp_failed=0, invalid=0, min_safety_ratio=np.inf, max_vel_excess=0.0, max_acc_excess=0.0, waypoints_updated=0,
                truncated_agent_steps=0, **(dict(safety_ratio_obs=np.inf) if n_dyn else {})) for k in range(missions)]
    for _ in range(steps):
        plan.step(graph=graph)
        torch.cuda.synchronize()
        st, valid, saf, upd, cnt = (plan.get(b) for b in (api.PLAN_STATUS, api.PLAN_VALID, api.PLAN_SAFETY, api.PLAN_WAYPOINT_UPDATED, api.PLAN_IN_RANGE))
        if n_dyn:
            fig = plan.get_obstacles(api.PLAN_OBS_SAFETY)["safety_ratio_obs"]
            min_obstacle_ratio = float(min(min_obstacle_ratio, fig.min()))
        for k, m in enumerate(per):
            sl = slice(int(off[k]), int(off[k + 1]))
            if n_dyn:  # (+inf: the mission has no obstacle of its own)
                m["safety_ratio_obs"] = float(min(m["safety_ratio_obs"], fig[sl].min()))
            m["qp_failed"] += int((st[sl] != 0).sum())
            m["invalid"] += int(((st[sl] == 0) & (valid[sl] != 1)).sum())
            m["min_safety_ratio"] = float(min(m["min_safety_ratio"], saf["safety_ratio"][sl].min()))
            m["max_vel_excess"] = float(max(m["max_vel_excess"], saf["vel_excess_ratio"][sl].max()))
            m["max_acc_excess"] = float(max(m["max_acc_excess"], saf["acc_excess_ratio"][sl].max()))
            m["waypoints_updated"] += int(upd[sl].sum())
            m["truncated_agent_steps"] += int((cnt[sl] > n_obs - n_slot).sum())
    state = plan.get(api.PLAN_STATE).reshape(N, 9)
    progress = np.linalg.norm(goals[:, :2] - starts[:, :2], axis=1) - np.linalg.norm(goals[:, :2] - state[:, :2], axis=1)
    status = plan.mission_status()
    for k, m in enumerate(per):
        m["mean_progress_m"] = float(progress[int(off[k]):int(off[k + 1])].mean())
        m["walk_bound_reached"] = int(status[k])
    if patrol is not None:
        legs = plan.patrol(api.PATROL_LEGS)
        for k, m in enumerate(per):
            m["legs"] = [int(v) for v in legs[int(off[k]):int(off[k + 1])]]
    log = dict(steps=steps, missions=missions, agents=N, row_slots=n_obs, router="device", sim_time_s=steps * dt, graph_nodes=plan.graph_nodes(),
               qp_failed=sum(m["qp_failed"] for m in per), invalid=sum(m["invalid"] for m in per),
               min_safety_ratio=min(m["min_safety_ratio"] for m in per), per_mission=per)
    if patrol is not None:
        log.update(patrol_goal_threshold=float(patrol), legs=sum(sum(m["legs"]) for m in per))
    if n_dyn:
        log.update(obstacles=n_dyn, obstacle_slots=n_slot, obstacles_per_mission=mission_obstacles is not None, driven_obstacles=n_driven,
                   min_obstacle_safety_ratio=min_obstacle_ratio)
    if world_set:
        log["worlds"] = len(world_set)
    plan.close()
    if world_set:
        world_set.close()
    for m_ in maps:
        m_.close()
    return log


def run(world_json, steps=40, M=10, dt=0.2, verbose=False, dump=None, keep_step=None, n_obs=None, script=None, router="host", missions=None,
        decision="one", until_finished=None, obstacles=None, worlds=None, obstacle_rows="lsc", log_csv=None, obstacle_specs=None, obstacle_seed=0,
        patrol=None, mission_obstacles=None, mission_obstacle_specs=None):
    """script (optional): {"waypoint": (K, N, 3), "state": (K, N, 9)} -- replay of a recorded mission: replan k takes every agent's
    state and waypoint from the script instead of the loop's own step / router (the plans, goal points, corridors and neighbour sets are
    still the loop's own), and the result carries every replan's solution (`x`, (K, N, nv)) and goal point (`goal`, (K, N, 3)).
    router: "host" (GridRouter) or "device" (lscqp_waypoints_device over the previous plans, states and goal points).
    missions: K > 0 flies K seeded missions over the world in one lscqp_plan (run_missions) and reports per-mission figures.
    decision (router "device"): "one" (lscqp_waypoints_device), "wide" (lscqp_waypoints_wide_device) or "auto" (wide from
    DECISION_AUTO_MIN_AGENTS agents on); the flight is the same whichever is chosen.
    until_finished (with missions): fly until every mission has finished, at most that many replans (run_missions).
    mission_obstacles, mission_obstacle_specs (with missions): a list of obstacles per mission, each mission's own (run_missions).
    obstacles (with missions): dynamic obstacles flown by the plan's own chain (load_obstacles, run_missions); obstacle_rows "lsc" or "clsc":
    the generator of their rows, and with it the plan's constraint mode (run_missions).  obstacle_specs, obstacle_seed: the file's entries
    (load_obstacle_specs) -- its chasing and gaussian obstacles are then driven on the device instead of being HELD at their start.
    worlds (with missions): one world per mission -- a directory of world CSVs, a list of CSV paths or of box lists (load_worlds, run_missions).
    log_csv (with until_finished): a directory for every mission's result log in the reference's format, from the device's flight log.
    patrol = T: a patrol with goal_threshold T flown by one lscqp_plan (run_missions; missions defaults to 1): legs per agent, per mission."""
    if patrol is not None and not missions:
        missions = 1
    if router not in ("host", "device"):
        raise ValueError("router must be 'host' or 'device'")
    if decision not in ("one", "wide", "auto"):
        raise ValueError("decision must be 'one', 'wide' or 'auto'")
    if until_finished and not missions:
        raise ValueError("until_finished needs missions=K (one lscqp_plan with a mission record)")
    if mission_obstacles is not None and not missions:
        raise ValueError("mission_obstacles need missions=K: list k belongs to mission k of an lscqp_plan (lscqp_plan_set_mission_obstacles)")
    if obstacles is not None and not missions:
        raise ValueError("obstacles need missions=K (K >= 1): they fly in the chain of an lscqp_plan (lscqp_plan_set_obstacles)")
    if worlds is not None and not missions:
        raise ValueError("worlds need missions=K: world k belongs to mission k of an lscqp_plan (lscqp_plan_set_worlds)")
    if log_csv and not until_finished:
        raise ValueError("log_csv needs until_finished=MAX with missions=K: the log is the plan's flight log, MAX rows per mission")
    if missions:
        return run_missions(world_json, int(missions), steps=steps, M=M, dt=dt, n_obs=n_obs, until_finished=until_finished, obstacles=obstacles,
                            worlds=worlds, obstacle_rows=obstacle_rows, log_csv=log_csv, obstacle_specs=obstacle_specs, obstacle_seed=obstacle_seed,
                            patrol=patrol, mission_obstacles=mission_obstacles, mission_obstacle_specs=mission_obstacle_specs,
                            **({} if patrol is None else {"goal_threshold": float(patrol)}))
    import torch

    from lsc_dr_planner_amd import api

    g = world_json if isinstance(world_json, dict) else json.load(open(world_json))
    dev = torch.device("cuda", 0)
    dim, z2d, radius = 2, float(g["z_2d"]), float(g["radius"])
    starts, desired = np.array(g["starts"], dtype=np.float64), np.array(g["goals"], dtype=np.float64)
    N = len(starts)
    # Row slots per agent.  The reference hands EVERY in-range agent to the planner (src/multi_sync_simulator.cpp:318-333), so the
    # slots follow the largest in-range count seen (lscqp_select_neighbours_device reports it) up to the largest compiled kernel
    # instance of the shape (lscqp_max_obstacles); only beyond that are the nearest kept, and that is counted in the result
    # (`truncated_agent_steps`) instead of happening silently.
    sol = api.Solver(api.make_desc(M=M, dim=dim, dt=dt, world_min=g["world_min"], world_max=g["world_max"]))
    cap = sol.max_obstacles()
    n_obs = min(N - 1, 8) if n_obs is None else n_obs
    n_obs = max(1, min(n_obs, cap))
    wmap = api.WorldMap(g["boxes"], g["world_min"], g["world_max"], g["resolution"], g["max_dist"])
    wmap.prepare(radius)  # the corridor kernel's free-space table (same boxes, tests in open space pass without sampling)
    nv = sol.nv
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    upb = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731

    # neighbours: chosen on the device each replan, the other agents within the communication range of the launch file (3 m)
    def row_buffers(k):
        return (torch.full((N * k,), -1, dtype=torch.int32, device=dev), up((np.arange(N + 1) * k * M * 6).astype(np.uint64).view(np.int64)),
                torch.zeros(N * k * M * 6 * 4, dtype=torch.float64, device=dev))

    d_nbr, d_off, d_rows = row_buffers(n_obs)
    d_ncount = torch.zeros(N, dtype=torch.int32, device=dev)
    comm_range = 3.0
    d_rad = torch.full((N,), radius, dtype=torch.float64, device=dev)
    d_dw = torch.full((N,), 2.0, dtype=torch.float64, device=dev)
    d_traj = torch.zeros(N * M * 6 * 3, dtype=torch.float64, device=dev)
    d_sfc = torch.zeros(N * M * 6, dtype=torch.float64, device=dev)
    d_sst = torch.zeros(N, dtype=torch.int32, device=dev)
    d_gst = torch.zeros(N, dtype=torch.int32, device=dev)
    d_qst = torch.zeros(N, dtype=torch.int32, device=dev)
    d_x = torch.zeros(N * nv, dtype=torch.float64, device=dev)
    d_obj = torch.zeros(N, dtype=torch.float64, device=dev)
    d_valid = torch.zeros(N, dtype=torch.int32, device=dev)
    d_state = torch.zeros(N * 9, dtype=torch.float64, device=dev)
    d_saf = torch.zeros(N * api.SAFETY_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    # t = 0: hover plans at the start points, corridors from initializeSFC
    state = np.zeros((N, 9))
    state[:, :3] = starts
    x_plan = np.zeros((N, dim, M, 6))
    for k in range(dim):
        x_plan[:, k] = starts[:, k, None, None]
    d_xprev = up(x_plan.reshape(N, -1))
    P0 = np.repeat(starts[:, None, :], 3, axis=1)
    sol.construct_sfc_device(wmap, api.SFC_INIT, N, up(P0.reshape(-1)), d_rad, d_sfc, d_sst)
    torch.cuda.synchronize()
    assert (d_sst.cpu().numpy() == 1).all(), "a start point lies inside an inflated obstacle"

    use_device_router = router == "device" and script is None
    grid_router = GridRouter(g, wmap.download()[0], wmap.key0) if script is None and not use_device_router else None
    if use_device_router:  # the grid planner's grid and the mission's distance fields, once
        grid = api.Grid(wmap, 0.5, radius, z2d)
        d_field, d_init_d = grid.fields(up(starts), up(desired))
        d_way = up(np.float32(starts).astype(np.float64))
        updated_total = 0
        use_wide = decision == "wide" or (decision == "auto" and N >= api.DECISION_AUTO_MIN_AGENTS)
        decide = grid.waypoints_wide if use_wide else grid.waypoints
    waypoint = starts.copy()  # first waypoint: the start node itself; it advances in the loop
    goal_pt = starts.copy()   # agent.current_goal_point
    log = {"steps": steps, "agents": N, "qp_failed": 0, "invalid": 0, "sfc_kept": 0, "goal_infeasible": 0, "min_safety_ratio": np.inf,
           "max_vel_excess": 0.0, "max_acc_excess": 0.0, "iters": []}
    d_info = torch.zeros(N * api.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    dist0 = np.linalg.norm(desired[:, :2] - starts[:, :2], axis=1)
    for step in range(steps):
        # initial trajectories of this replan: the previous plans shifted by one segment (none before the first solve)
        sol.shift_traj_device(N, d_xprev, d_traj, z_2d=z2d, shift=0 if step == 0 else 1)
        torch.cuda.synchronize()
        traj = d_traj.cpu().numpy().reshape(N, M, 6, 3)
        last = traj[:, M - 1, 5]
        # the waypoint advances to the next node of the grid path once the agent is close to the current one (the reference's
        # planner hands out one grid step at a time, which keeps the QP's communication-range rows |x - waypoint| <= R/2
        # satisfiable); the current goal point is the outcome of the previous goal LP (src/traj_planner.cpp:545-549)
        if script is not None:
            state, waypoint = np.array(script["state"][step], dtype=np.float64), np.array(script["waypoint"][step], dtype=np.float64)
        elif use_device_router:
            # decentralizedMAPP: one PIBT step per communication group from the plans as the last replan left them, then the update filter
            _, _, d_upd = decide(comm_range, M, dim, up(state), d_xprev, up(goal_pt), d_field, d_init_d, d_way)
            waypoint = d_way.cpu().numpy().reshape(N, 3)
            updated_total += int(d_upd.sum().item())
        else:
            for a in range(N):
                if np.abs(state[a, :2] - waypoint[a, :2]).max() < 0.3:
                    waypoint[a, :2] = grid_router.next_waypoint(waypoint[a], desired[a])[0]
        waypoint = np.float32(waypoint).astype(np.float64)
        if step > 0:
            P = np.stack([last, goal_pt, waypoint], axis=1)
            sol.construct_sfc_device(wmap, api.SFC_FROM_HULL, N, up(P.reshape(-1)), d_rad, d_sfc, d_sst)
        d_goal_all = up(goal_pt)
        sol.select_neighbours_device(N, 0, N, n_obs, comm_range, up(state[:, :3]), d_nbr, d_ncount)  # broadcastMsgs' range filter
        need = int(d_ncount.max().item())
        if need > n_obs and n_obs < cap:  # more agents in range than slots: grow the row buffers and select again
            n_obs = min(need, cap)
            d_nbr, d_off, d_rows = row_buffers(n_obs)
            sol.select_neighbours_device(N, 0, N, n_obs, comm_range, up(state[:, :3]), d_nbr, d_ncount)
        log["row_slots"] = n_obs
        log["truncated_agent_steps"] = log.get("truncated_agent_steps", 0) + int((d_ncount > n_obs).sum().item())
        sol.generate_constraints_device(api.GEN_CLSC, N, n_obs, 0, d_traj, d_nbr, d_rad, d_dw, d_goal_all, d_rows)
        hdr = np.zeros(N, api.HEADER_DTYPE)
        hdr["p0"], hdr["v0"], hdr["a0"] = state[:, 0:3], state[:, 3:6], state[:, 6:9]
        hdr["goal"], hdr["next_waypoint"] = goal_pt, waypoint
        hdr["vmax"], hdr["amax"], hdr["radius"], hdr["nominal_velocity"], hdr["n_obs"] = 1.0, 2.0, radius, 1.0, n_obs
        d_hdr = upb(hdr)
        sol.optimize_goal_device(N, d_hdr, d_rows, d_off, d_sfc, d_gst)
        # x_init: the shifted plan in the solver's layout
        x_init = np.ascontiguousarray(traj.transpose(0, 3, 1, 2)[:, :dim].reshape(N, -1))
        d_xinit = up(x_init)
        sol.solve_device(N, n_obs, d_hdr, d_rows, d_off, d_sfc, d_x, d_obj, d_qst, d_info=d_info, d_x_init=d_xinit)
        sol.validate_step_device(N, dt, d_x, d_hdr, d_sfc, d_valid, d_state, z_2d=z2d)
        torch.cuda.synchronize()
        qst, valid = d_qst.cpu().numpy(), d_valid.cpu().numpy()
        if ((qst == 2) | (qst == 3)).any():
            # a warm-started iteration that ran out of iterations or broke down: one cold re-launch of the batch, results taken
            # for those agents only (what the host entry point lscqp_solve_batch does by itself)
            d_x2, d_obj2, d_st2 = torch.zeros_like(d_x), torch.zeros_like(d_obj), torch.zeros_like(d_qst)
            sol.solve_device(N, n_obs, d_hdr, d_rows, d_off, d_sfc, d_x2, d_obj2, d_st2)
            torch.cuda.synchronize()
            st2 = d_st2.cpu().numpy()
            fix = ((qst == 2) | (qst == 3)) & (st2 == 0)
            if fix.any():
                sel = torch.from_numpy(np.nonzero(fix)[0]).to(dev)
                d_x.view(N, nv)[sel] = d_x2.view(N, nv)[sel]
                d_obj[sel] = d_obj2[sel]
                d_qst[sel] = d_st2[sel]
                log["cold_retries"] = log.get("cold_retries", 0) + int(fix.sum())
                sol.validate_step_device(N, dt, d_x, d_hdr, d_sfc, d_valid, d_state, z_2d=z2d)
                torch.cuda.synchronize()
                qst, valid = d_qst.cpu().numpy(), d_valid.cpu().numpy()
        good = (qst == 0) & (valid == 1)
        x_new = d_x.cpu().numpy().reshape(N, nv)
        if keep_step is not None and step == keep_step:  # inputs and outputs of one replan, for the parity test
            log["kept"] = dict(hdr=d_hdr.cpu().numpy().view(api.HEADER_DTYPE).copy(), rows=d_rows.cpu().numpy().view(api.ROW_DTYPE).copy(),
                               sfc=d_sfc.cpu().numpy().view(api.BOX_DTYPE).reshape(N, M).copy(), x=d_x.cpu().numpy().reshape(N, nv).copy(),
                               obj=d_obj.cpu().numpy().copy(), status=qst.copy(), n_obs=n_obs, world_min=g["world_min"], world_max=g["world_max"])
        if dump and (qst != 0).any() and not os.path.exists(dump):
            np.savez(dump, hdr=d_hdr.cpu().numpy(), rows=d_rows.cpu().numpy(), sfc=d_sfc.cpu().numpy(), qst=qst, x_init=x_init,
                     info=d_info.cpu().numpy(), step=step)
        if not good.all():  # the reference substitutes the initial trajectory (src/traj_planner.cpp:767-797)
            x_new[~good] = x_init[~good]
            d_x.copy_(up(x_new.reshape(-1)))
            sol.validate_step_device(N, dt, d_x, d_hdr, d_sfc, d_valid, d_state, z_2d=z2d)
        sol.safety_metrics_device(N, 0, N, 2, 0.1, d_x, d_rad, d_dw, d_hdr, d_saf, z_2d=z2d)
        torch.cuda.synchronize()
        saf = d_saf.cpu().numpy().view(api.SAFETY_DTYPE)
        state = d_state.cpu().numpy().reshape(N, 9)
        d_xprev.copy_(d_x.view(N, nv))
        goal_pt = d_hdr.cpu().numpy().view(api.HEADER_DTYPE)["goal"].copy()  # the goal LP's result is the next current goal point
        if script is not None:
            log.setdefault("x", []).append(x_new.copy())
            log.setdefault("goal", []).append(goal_pt.copy())
            log.setdefault("n_in_range", []).append(d_ncount.cpu().numpy().copy())
        log["max_in_range"] = int(max(log.get("max_in_range", 0), d_ncount.cpu().numpy().max()))
        log["qp_failed"] += int((qst != 0).sum())
        log["invalid"] += int(((qst == 0) & (valid != 1)).sum())
        log["sfc_kept"] += int((d_sst.cpu().numpy() == 0).sum()) if step > 0 else 0
        log["goal_infeasible"] += int((d_gst.cpu().numpy() != 0).sum())
        log["min_safety_ratio"] = float(min(log["min_safety_ratio"], saf["safety_ratio"].min()))
        log["max_vel_excess"] = float(max(log["max_vel_excess"], saf["vel_excess_ratio"].max()))
        log["max_acc_excess"] = float(max(log["max_acc_excess"], saf["acc_excess_ratio"].max()))
        log["iters"].append(int(d_info.cpu().numpy().view(api.INFO_DTYPE)["iterations"].max()))
        if verbose:
            print(step, "failed", int((qst != 0).sum()), "invalid", int(((qst == 0) & (valid != 1)).sum()), "safety",
                  float(saf["safety_ratio"].min()), "dist", np.linalg.norm(desired[:, :2] - state[:, :2], axis=1).round(2), file=sys.stderr)
    dist1 = np.linalg.norm(desired[:, :2] - state[:, :2], axis=1)
    log["mean_progress_m"] = float((dist0 - dist1).mean())
    log["min_progress_m"] = float((dist0 - dist1).min())
    log["sim_time_s"] = steps * dt
    log["max_iters"] = int(max(log["iters"]))
    del log["iters"]
    # occupancy check of the flown positions: the agents (L-infinity radius) never touch an occupied cell
    log["router"] = router
    if use_device_router:
        log["decision"] = "wide" if use_wide else "one"
        log["waypoints_updated"] = updated_total
        assert grid.status() == 0
        grid.close()
    wmap.close()
    return log


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--world", default=os.path.join(ROOT, "tests", "golden", "forest10_world.json"))
    ap.add_argument("-v", action="store_true")
    ap.add_argument("--forest", type=int, default=0, help="N > 0: a synthetic forest with N agents instead of --world")
    ap.add_argument("--obs", type=int, default=None, help="neighbour capacity per agent")
    ap.add_argument("--dump", default=None, help="npz path: inputs of the first replan with a failed QP")
    ap.add_argument("--missions", type=int, default=0, help="K > 0: K seeded missions over the world in ONE plan with a mission partition, figures per mission")
    ap.add_argument("--until-finished", type=int, nargs="?", const=400, default=None, metavar="MAX",
                    help="with --missions K: fly until every mission has finished (lscqp_plan_run over the plan's mission record), at most MAX replans (default 400); "
                         "one record per mission")
    ap.add_argument("--decision", default="one", choices=("one", "wide", "auto"),
                    help="with --router device: the one-workgroup decision, lscqp_waypoints_wide_device, or wide from DECISION_AUTO_MIN_AGENTS agents on")
    ap.add_argument("--obstacles", default=None, nargs="+", metavar="FILE.json",
                    help="with --missions K: the dynamic obstacles of a reference mission file (its \"obstacles\" list, or a bare list: type, start, goal, "
                         "waypoints, axis, size, speed, max_acc, downwash), moved by the plan's chain.  One file: shared by every mission.  K files: "
                         "mission k flies among the obstacles of file k and sees no other's (a chaser's target_agent counts from its mission's first agent)")
    ap.add_argument("--obstacle-rows", default="lsc", choices=("lsc", "clsc"),
                    help="with --obstacles: lsc = generateLSC's rows for obstacles and agents alike (the plan flies GEN_LSC); clsc = the plan keeps "
                         "GEN_CLSC, the reference's launch mode, and the obstacles get generateCLSC's rows")
    ap.add_argument("--drive-obstacles", action="store_true",
                    help="with --obstacles: the file's chasing and gaussian obstacles move on the device, inside the chain (without it they are "
                         "held at their start)")
    ap.add_argument("--obstacle-seed", type=int, default=0, help="with --drive-obstacles: seed of the gaussian obstacles' acceleration histories")
    ap.add_argument("--worlds", default=None, nargs="+", metavar="CSV",
                    help="with --missions K: K world CSVs (or one directory holding K) in the world's box -- mission k flies over world k, as "
                         "launch/test_all_*.launch pair a mission directory with a world directory")
    ap.add_argument("--log-csv", default=None, metavar="DIR",
                    help="with --until-finished: keep the flight log on the device and write every mission's result log in the reference's format to DIR/mission_<k>.csv")
    ap.add_argument("--patrol", action="store_true",
                    help="fly a patrol for --steps replans (lscqp_plan_set_patrol): every agent swaps start and goal on arrival; prints the legs per "
                         "agent, with --missions K per mission")
    ap.add_argument("--goal-threshold", type=float, default=0.1, metavar="T", help="with --patrol: the arrival threshold (the launch files' 0.1)")
    ap.add_argument("--router", default="host", choices=("host", "device"), help="where the waypoints come from: the host stand-in or lscqp_waypoints_device")
    a = ap.parse_args()
    world = random_forest_world(a.forest) if a.forest > 0 else a.world
    shared = a.obstacles[0] if a.obstacles and len(a.obstacles) == 1 else None
    own = a.obstacles if a.obstacles and len(a.obstacles) > 1 else None
    if own and len(own) != a.missions:
        ap.error("--obstacles: one file (shared by every mission) or one per mission -- %d files for --missions %d" % (len(own), a.missions))
    print(json.dumps(run(world, steps=a.steps, verbose=a.v, dump=a.dump, n_obs=a.obs, router=a.router, missions=a.missions, decision=a.decision,
                         until_finished=a.until_finished, obstacles=load_obstacles(shared) if shared else None, worlds=a.worlds,
                         obstacle_rows=a.obstacle_rows, log_csv=a.log_csv,
                         obstacle_specs=load_obstacle_specs(shared) if shared and a.drive_obstacles else None, obstacle_seed=a.obstacle_seed,
                         patrol=a.goal_threshold if a.patrol else None, mission_obstacles=[load_obstacles(f) for f in own] if own else None,
                         mission_obstacle_specs=[load_obstacle_specs(f) for f in own] if own and a.drive_obstacles else None)))
