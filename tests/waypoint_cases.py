"""Inputs shared by tests/test_grid_reference.py (CPU: the restatement against known answers) and tests/test_waypoints_gpu.py (the device
against the restatement): toy worlds with hand-worked PIBT outcomes, seeded missions on random forests, seeded states along a rollout."""
import json
import os

import numpy as np

from tests import grid_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = 0.5


def forest10():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))


def toy_world(rows):
    """rows: strings, '.' = free node, '#' = occupied, rows[0] is y = 1 (a ring of occupied nodes surrounds the picture).  Nodes lie 0.5 m apart;
    an occupied node carries a 0.2 m pillar, which the occupancy rule (radius 0.15) turns into exactly that node."""
    H, W = len(rows) + 2, len(rows[0]) + 2
    occ = np.ones((H, W), bool)
    for j, r in enumerate(rows):
        for i, c in enumerate(r):
            occ[j + 1, i + 1] = c == "#"
    boxes = [[0.5 * i, 0.5 * j, 0.5, 0.2, 0.2, 1.0] for j in range(H) for i in range(W) if occ[j, i]]
    return {"boxes": boxes, "world_min": [0.0, 0.0, 0.0], "world_max": [0.5 * (W - 1), 0.5 * (H - 1), 1.0], "resolution": 0.1, "max_dist": 1.0,
            "z_2d": Z, "radius": 0.15, "occ": occ}


def P(i, j):  # the point of picture node (i, j)
    return [0.5 * (i + 1), 0.5 * (j + 1), Z]


def N(i, j, W):  # ... and its node id in a picture W wide
    return (j + 1) * (W + 2) + (i + 1)


# name -> (rows, waypoints, goals, init_d or None (= from the starts, which are the waypoints), positions or None (= waypoints), range,
#          expected desired picture nodes).  The higher id wins a priority tie (tie_breaker = id / n).
TOYS = {
    # A (init_d 3 against 2: the priority) wants B's node; B cannot swap and cannot stay, so it backs off to the right: priority inheritance
    "head_on": (["....."], [P(1, 0), P(2, 0)], [P(4, 0), P(0, 0)], None, None, -1, [(2, 0), (3, 0)]),
    # nowhere to back off to: the swap is refused and both stay
    "swap_refused": ([".."], [P(0, 0), P(1, 0)], [P(1, 0), P(0, 0)], None, None, -1, [(0, 0), (1, 0)]),
    # A sits in a dead end behind B, B's goal is A's node: A fails (stays), B replans and stays
    "dead_end": (["..."], [P(0, 0), P(1, 0)], [P(2, 0), P(0, 0)], [1, 2], None, -1, [(0, 0), (1, 0)]),
    # A rests on its goal in B's way: B (init_d 2) pushes it ahead (right comes before down in the identity order)
    "pushed_off_goal": (["...", "#.#"], [P(1, 0), P(0, 0)], [P(1, 0), P(2, 0)], [0, 2], None, -1, [(2, 0), (1, 0)]),
    # two agents out of each other's range head for the same node: each is alone in its group and takes it
    "two_groups": (["..."], [P(0, 0), P(2, 0)], [P(2, 0), P(0, 0)], None, [[0.5, 0.5, Z], [40.0, 0.5, Z]], 3.0, [(1, 0), (1, 0)]),
    # ... and as one group only the priority agent (id 1) gets it
    "one_group": (["..."], [P(0, 0), P(2, 0)], [P(2, 0), P(0, 0)], None, None, -1, [(0, 0), (1, 0)]),
    # range 0: nobody is within it, every agent is alone (and, as for a negative range, the filter has no range test)
    "range_zero": (["..."], [P(0, 0), P(2, 0)], [P(2, 0), P(0, 0)], None, None, 0.0, [(1, 0), (1, 0)]),
}


def toy_case(name):
    rows, way, goals, init_d, pos, rng, expect = TOYS[name]
    w = toy_world(rows)
    way, goals = np.array(way, float), np.array(goals, float)
    pos = way.copy() if pos is None else np.array(pos, float)
    return dict(world=w, starts=way.copy(), goals=goals, waypoints=way, positions=pos, current_goals=way.copy(), range=rng, init_d=init_d,
                expect=[N(i, j, len(rows[0])) for (i, j) in expect], plans=None)


def reference_grid(oracle, w, resolution=0.5):
    mp = oracle.Map(w["boxes"], w["world_min"], w["world_max"], w["resolution"], w["max_dist"])
    return R.Grid(w["world_min"], w["world_max"], w["z_2d"], resolution, w["radius"], mp.nearest(), mp.key0, w["resolution"])


def random_mission(n, side=40.0, n_boxes=300, seed=0):
    """n agents on distinct free nodes of a random forest (pillars 0.5 x 0.5 m) with distinct goal nodes, all on the 0.5 m grid."""
    rng = np.random.default_rng(seed)
    half = side / 2
    boxes = [[c[0], c[1], 1.25, 0.5, 0.5, 2.5] for c in rng.uniform(-half + 1, half - 1, (n_boxes, 2))]
    B = np.array(boxes)[:, :2]
    m = int(side / 0.5) - 3
    picks = []
    seen = set()
    while len(picks) < 2 * n:
        ij = tuple(rng.integers(2, m, 2))
        p = -half + 0.5 * np.array(ij)
        if ij in seen or np.abs(B - p).max(axis=1).min() < 0.8:
            continue
        seen.add(ij)
        picks.append([p[0], p[1], 0.6])
    return {"boxes": boxes, "world_min": [-half, -half, 0.0], "world_max": [half, half, 2.5], "resolution": 0.1, "max_dist": 1.0, "z_2d": 0.6,
            "radius": 0.15, "starts": picks[:n], "goals": picks[n:]}


def walled_world(nodes=400):
    """A grid too large for LDS: nodes x nodes, two long walls with gaps and one closed pocket that no path enters."""
    side = 0.5 * (nodes - 1)
    boxes = []
    for k, x in enumerate((0.25 * side, 0.6 * side)):
        gap = 0.2 * side if k == 0 else 0.8 * side
        boxes.append([x, (gap - 1.0) / 2, 1.0, 0.5, gap - 1.0, 2.0])
        boxes.append([x, (gap + 1.0 + side) / 2, 1.0, 0.5, side - gap - 1.0, 2.0])
    c = np.array([0.8 * side, 0.3 * side])  # the pocket: four walls around a 3 m square
    for dx, dy, sx, sy in ((0, 2.0, 4.5, 0.5), (0, -2.0, 4.5, 0.5), (2.0, 0, 0.5, 4.5), (-2.0, 0, 0.5, 4.5)):
        boxes.append([c[0] + dx, c[1] + dy, 1.0, sx, sy, 2.0])
    pocket = [float(np.round(c[0] / 0.5) * 0.5), float(np.round(c[1] / 0.5) * 0.5), 0.6]
    starts = [[1.0, 1.0, 0.6], [side - 1.0, side - 1.0, 0.6], [1.0, side - 1.0, 0.6]]
    goals = [[side - 1.0, 1.0, 0.6], [1.0, 1.0, 0.6], pocket]
    return {"boxes": boxes, "world_min": [0.0, 0.0, 0.0], "world_max": [side, side, 2.0], "resolution": 0.1, "max_dist": 1.0, "z_2d": 0.6,
            "radius": 0.15, "starts": starts, "goals": goals, "pocket": pocket}


def seeded_states(grid, w, fields, init_d, steps, rng_range, seed, M=10, jump=0.7):
    """States along a grid rollout of mission w, for the filter to have something to decide: per step a dict with positions (waypoint + noise),
    plan points (M + 1 points scattered around the position), current goal points (the waypoint for most agents, elsewhere for some) and the
    waypoints; the rollout advances by the restatement's own decision, and agents that were refused jump anyway now and then."""
    rnd = np.random.default_rng(seed)
    way = np.array(w["starts"], float)
    n = len(way)
    out = []
    for _ in range(steps):
        pos = way + np.c_[rnd.uniform(-0.2, 0.2, (n, 2)), np.zeros(n)]
        pos = np.float32(pos).astype(np.float64)
        spread = rnd.choice([0.1, 0.6, 1.2], n)
        pts = pos[:, None, :] + np.concatenate([rnd.uniform(-1, 1, (n, M + 1, 2)) * spread[:, None, None], np.zeros((n, M + 1, 1))], axis=2)
        pts = np.float32(pts).astype(np.float64)
        cg = way.copy()
        far = rnd.random(n) < 0.15
        cg[far, :2] += 0.25
        out.append(dict(positions=pos, plans=pts, current_goals=cg, waypoints=way.copy()))
        _, desired, _, new = R.waypoint_step(grid, rng_range, pos, list(pts), cg, way, fields, init_d)
        move = rnd.random(n) < jump
        for i in range(n):
            if move[i]:
                new[i] = grid.point((int(desired[i]) % grid.W, int(desired[i]) // grid.W))
        # (a forced jump may put two agents of different groups on one node; keep the nodes distinct, PIBT's own precondition)
        taken = {}
        for i in range(n):
            nd = grid.node(new[i])
            if nd in taken:
                new[i] = way[i]
                nd = grid.node(new[i])
            taken[nd] = i
        if len({grid.node(p) for p in new}) == n:
            way = np.array(new, float)
    return out


def plan_from_points(pts, dim=2):
    """The plan buffer layout x[k][m][i] whose segment start points and last point are pts (n, M + 1, 3); the other control points are fill."""
    n, M1, _ = pts.shape
    M = M1 - 1
    x = np.zeros((n, dim, M, 6))
    for k in range(dim):
        x[:, k, :, :] = pts[:, :M, k][:, :, None]
        x[:, k, M - 1, 5] = pts[:, M, k]
    return x.reshape(n, -1)
