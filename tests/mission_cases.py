"""Many missions over one map (include/lscqp.h, "many missions over one map"): the test-side restatement and its inputs, shared by
tests/test_missions_abi.py (CPU: the restatement against itself) and tests/test_missions_gpu.py (the device against the restatement).

The restatement is tests/grid_reference.py applied to each mission's slice with that mission's cleared nodes: missions share the grid's
static occupancy and nothing else.  Inputs: ONE forest and K start / goal sets drawn from seeds."""
import numpy as np

from tests import grid_reference as R
from tests import waypoint_cases as WC


def forest_missions(K, n=10, side=40.0, n_boxes=300, seed=0):
    """One random forest (pillars 0.5 x 0.5 m, drawn from `seed` alone) and K missions of n agents each: mission k's distinct free start and
    goal nodes are drawn from (seed, k) alone, so it is the same mission whatever K is.  Missions may share nodes with each other.
    Returns (world, offsets [K + 1], starts (K n, 3), goals (K n, 3)); the world has no starts / goals of its own."""
    half = side / 2
    boxes = [[c[0], c[1], 1.25, 0.5, 0.5, 2.5] for c in np.random.default_rng(seed).uniform(-half + 1, half - 1, (n_boxes, 2))]
    B = np.array(boxes)[:, :2]
    m = int(side / 0.5) - 3
    starts, goals = [], []
    for k in range(K):
        rng = np.random.default_rng([seed, k])
        picks, seen = [], set()
        while len(picks) < 2 * n:
            ij = tuple(int(v) for v in rng.integers(2, m, 2))
            p = -half + 0.5 * np.array(ij)
            if ij in seen or np.abs(B - p).max(axis=1).min() < 0.8:
                continue
            seen.add(ij)
            picks.append([p[0], p[1], 0.6])
        starts += picks[:n]
        goals += picks[n:]
    world = {"boxes": boxes, "world_min": [-half, -half, 0.0], "world_max": [half, half, 2.5], "resolution": 0.1, "max_dist": 1.0, "z_2d": 0.6,
             "radius": 0.15}
    return world, np.arange(K + 1) * n, np.array(starts, float), np.array(goals, float)


def slices(offsets):
    return [slice(int(offsets[k]), int(offsets[k + 1])) for k in range(len(offsets) - 1)]


def mission_fields(G, offsets, starts, goals):
    """R.mission_fields per mission.  Returns (fields (n, H, W), init_d (n,), free: per mission the graph of that mission -- the static
    occupancy with ITS start and goal nodes cleared)."""
    F, D, free = [], [], []
    for sl in slices(offsets):
        f, d = R.mission_fields(G, list(starts[sl]), list(goals[sl]))
        F.append(f)
        D.append(d)
        free.append(G.free.copy())
    return np.concatenate(F), np.concatenate(D), free


def waypoint_step(G, free, offsets, rng, positions, plans_pts, current_goals, waypoints, fields, init_d):
    """R.waypoint_step per mission on that mission's graph; group labels are global ids (offset + the slice's own label)."""
    out = [[], [], [], []]
    for k, sl in enumerate(slices(offsets)):
        G.free = free[k]
        pl = None if plans_pts is None else list(plans_pts[sl])
        label, desired, updated, way = R.waypoint_step(G, rng, positions[sl], pl, current_goals[sl], waypoints[sl], fields[sl], init_d[sl])
        for o, v in zip(out, (label + int(offsets[k]), desired, updated, way)):
            o.append(v)
    return tuple(np.concatenate(o) for o in out)


def seeded_states(G, free, offsets, world, starts, fields, init_d, steps, rng, seed):
    """WC.seeded_states per mission (seed + k), joined step by step."""
    per = []
    for k, sl in enumerate(slices(offsets)):
        G.free = free[k]
        w = dict(world, starts=[list(p) for p in starts[sl]])
        per.append(WC.seeded_states(G, w, fields[sl], init_d[sl], steps, rng, seed + k))
    return [{key: np.concatenate([p[t][key] for p in per]) for key in per[0][t]} for t in range(steps)]
