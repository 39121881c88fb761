"""Each mission over its own world (include/lscqp.h, "each mission over its own world"): the inputs and the test-side restatement shared by
tests/test_worlds_cpu.py, tests/test_worlds_gpu.py and tests/test_worlds_plan_gpu.py.

The fixture tests/golden/forest_worlds.json holds the first four worlds of the reference's forest set -- one box, one resolution, different
pillars -- and the agents of the mission that goes with the first.  The restatement is tests/grid_reference.py applied to each mission's
slice over that mission's OWN occupancy: with worlds, missions share the grid's shape and nothing else."""
import json
import os

import numpy as np

from tests import grid_reference as R
from tests import waypoint_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WORLDS = 4


def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "forest_worlds.json")))


def world(k, g=None):
    """World k of the fixture in the shape the other cases use (boxes, world box, resolution, ...); world 0 carries the fixture's agents."""
    g = fixture() if g is None else g
    w = {key: g[key] for key in ("world_min", "world_max", "resolution", "max_dist", "z_2d", "radius")}
    w["boxes"] = g["worlds"][k]
    if k == 0:
        w["starts"], w["goals"] = g["starts"], g["goals"]
    return w


def seeded_nodes(n, seed, g=None):
    """n distinct nodes of the 0.5 m grid inside the world box (one node off its border), at z = z_2d, drawn from `seed`; occupied ones included."""
    g = fixture() if g is None else g
    lo, hi = np.array(g["world_min"][:2]) + 0.5, np.array(g["world_max"][:2]) - 0.5
    nx, ny = (np.round((hi - lo) / 0.5).astype(int) + 1).tolist()
    assert n <= nx * ny
    pick = np.random.default_rng(seed).choice(nx * ny, size=n, replace=False)
    return np.c_[lo[0] + 0.5 * (pick % nx), lo[1] + 0.5 * (pick // nx), np.full(n, float(g["z_2d"]))]


def free_nodes(boxes, n, seed, g=None, clearance=0.8):
    """n distinct grid nodes at least `clearance` (L-infinity) from every pillar centre of `boxes`, drawn from `seed`: free in that world's grid."""
    g = fixture() if g is None else g
    B = np.asarray(boxes, float)[:, :2]
    out = [p for p in seeded_nodes(19 * 19, seed, g) if np.abs(B - p[:2]).max(axis=1).min() >= clearance]
    assert len(out) >= n
    return np.array(out[:n])


def seeded_missions(sizes, seed=0, g=None, free_everywhere=False):
    """Missions of the given sizes, mission k over world k of the fixture: mission 0 is the fixture's own agents (the first sizes[0] of them),
    mission k > 0 has distinct start and distinct goal nodes free in world k -- free_everywhere: in every world of the missions, world 0
    included, so that the same agents can also fly over ONE map --, drawn from (seed, k).  (offsets, starts, goals)."""
    g = fixture() if g is None else g
    starts, goals = [], []
    for k, n in enumerate(sizes):
        if k == 0:
            s, t = np.array(g["starts"], float)[:n], np.array(g["goals"], float)[:n]
            s[:, 2] = t[:, 2] = g["z_2d"]
        else:
            boxes = sum((g["worlds"][j] for j in range(len(sizes))), []) if free_everywhere else g["worlds"][k]
            p = free_nodes(boxes, 2 * n, [seed, k], g)
            s, t = p[:n], p[n:]
        starts.append(s)
        goals.append(t)
    return np.concatenate([[0], np.cumsum(sizes)]), np.concatenate(starts), np.concatenate(goals)


def synthetic_worlds(K, side=40.0, n_boxes=300, seed=0):
    """K random forests of one shape on a `side` m square (pillars as tests/mission_cases.py draws them), forest k from (seed, k)."""
    half = side / 2
    base = {"world_min": [-half, -half, 0.0], "world_max": [half, half, 2.5], "resolution": 0.1, "max_dist": 1.0, "z_2d": 0.6, "radius": 0.15}
    out = []
    for k in range(K):
        c = np.random.default_rng([seed, k]).uniform(-half + 1, half - 1, (n_boxes, 2))
        out.append(dict(base, boxes=[[x, y, 1.25, 0.5, 0.5, 2.5] for x, y in c]))
    return out


def slices(offsets):
    return [slice(int(offsets[k]), int(offsets[k + 1])) for k in range(len(offsets) - 1)]


def reference_grids(w, occs, resolution=0.5):
    """One restatement grid per mission from that mission's base occupancy (the rule that makes an occupancy is tested where one map is)."""
    return [R.Grid(w["world_min"], w["world_max"], w["z_2d"], resolution, w["radius"], occ=np.asarray(o).astype(bool)) for o in occs]


def mission_fields(Gs, offsets, starts, goals):
    """R.mission_fields per mission on its own grid (which keeps the mission's graph: start and goal nodes cleared).  (fields, init_d)"""
    F, D = [], []
    for G, sl in zip(Gs, slices(offsets)):
        f, d = R.mission_fields(G, list(starts[sl]), list(goals[sl]))
        F.append(f)
        D.append(d)
    return np.concatenate(F), np.concatenate(D)


def waypoint_step(Gs, offsets, rng, positions, plans_pts, current_goals, waypoints, fields, init_d):
    """R.waypoint_step per mission on its own grid; group labels are global ids."""
    out = [[], [], [], []]
    for k, (G, sl) in enumerate(zip(Gs, slices(offsets))):
        pl = None if plans_pts is None else list(plans_pts[sl])
        label, desired, updated, way = R.waypoint_step(G, rng, positions[sl], pl, current_goals[sl], waypoints[sl], fields[sl], init_d[sl])
        for o, v in zip(out, (label + int(offsets[k]), desired, updated, way)):
            o.append(v)
    return tuple(np.concatenate(o) for o in out)


def seeded_states(Gs, offsets, w, starts, fields, init_d, steps, rng, seed):
    """WC.seeded_states per mission (seed + k) on its own grid, joined step by step."""
    per = []
    for k, (G, sl) in enumerate(zip(Gs, slices(offsets))):
        per.append(WC.seeded_states(G, dict(w, starts=[list(p) for p in starts[sl]]), fields[sl], init_d[sl], steps, rng, seed + k))
    return [{key: np.concatenate([p[t][key] for p in per]) for key in per[0][t]} for t in range(steps)]
