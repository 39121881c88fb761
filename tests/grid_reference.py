"""Plain Python restatement of the reference's grid planner / MAPF step, written from its source: the test-side reference of
lscqp_grid and lscqp_waypoints_device (include/lscqp.h, "the grid planner / MAPF layer").

    GridBasedPlanner::updateGridInfo / updateGridMap / updateGridMission      src/grid_based_planner.cpp:86-140, 255-283
    Grid::Grid (x-y, 4-connected: left, right, up, down)                       third_party/grid-pathfinding/graph/src/graph.cpp:371-400
    Solver::createDistanceTable (a queue BFS from each goal)                   src/mapf/solver.cpp:270-289
    PIBT::run, first timestep; funcPIBT (recursive), planOneStep, chooseNode   src/mapf/pibt.cpp
    MultiSyncSimulator::decentralizedMAPP: groups, the update filter           src/multi_sync_simulator.cpp:160-303

with the three documented differences of the product: start and goal nodes of every agent of the mission are cleared once (not per
group and replan), chooseNode visits its candidates in the identity order left, right, up, down, stay instead of a shuffled one, and
only the first timestep of PIBT exists (no repeated leading configurations to drop, no "MAPF failed").  Nothing here shares code with
the product: a deque BFS where the kernel relaxes in sweeps, recursion where it keeps a stack, Python sets and the reference's literal
"find valid update" loop where it propagates flags.
"""
import collections
import math
import sys

import numpy as np

UNREACHABLE = 0x3FFFFFFF
EPS = 1e-9         # SP_EPSILON
EPS_FLOAT = 1e-5   # SP_EPSILON_FLOAT
f32 = np.float32


def c_round(x):  # C's round(): halves away from zero
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def grid_shape(world_min, world_max, resolution, world_dimension=2, z_2d=0.0):
    """updateGridInfo (:86-100) -> (grid_min [3], dims [3])."""
    gmin = [-math.floor((-float(world_min[i]) + EPS) / resolution) * resolution for i in range(3)]
    gmax = [math.floor((float(world_max[i]) + EPS) / resolution) * resolution for i in range(3)]
    if world_dimension == 2:
        gmin[2] = gmax[2] = z_2d
    dims = [c_round((gmax[i] - gmin[i]) / resolution) + 1 for i in range(3)]
    return gmin, dims


class Grid:
    """The 2-D grid of a mission.  nearest / key0 / map_dims / map_res: the voxel map's nearest-occupied-cell field
    (oracle.Map(...).nearest(), codes (dx+128) | (dy+128)<<8 | (dz+128)<<16 | 1<<24, 0 = none within max_dist)."""

    def __init__(self, world_min, world_max, z_2d, resolution=0.5, radius=0.15, nearest=None, key0=None, map_res=0.1, occ=None):
        # (mission.world_min / world_max are point3d: float32)
        self.res, self.z_2d, self.radius = float(resolution), float(z_2d), float(radius)
        self.gmin, self.dims = grid_shape([float(f32(v)) for v in world_min], [float(f32(v)) for v in world_max], self.res, 2, self.z_2d)
        self.W, self.H = self.dims[0], self.dims[1]
        if occ is not None:  # a hand-made grid (toy cases): occ[y][x]
            self.occ = np.array(occ, dtype=bool).copy()
            assert self.occ.shape == (self.H, self.W)
        else:
            self.occ = np.zeros((self.H, self.W), bool)
            for j in range(self.H):
                for i in range(self.W):
                    self.occ[j, i] = self._occupied(self.point((i, j)), nearest, key0, float(map_res))
        self.free = ~self.occ  # the mission's graph: clear() opens start and goal nodes

    def point(self, node):
        """gridNodeToPoint3D (:386-399): a point3d."""
        return np.array([f32(self.gmin[0] + node[0] * self.res), f32(self.gmin[1] + node[1] * self.res), f32(self.z_2d)], dtype=f32)

    def node(self, p):
        """point3DToGridVector (:429-441), x and y."""
        out = []
        for k in range(2):
            v = c_round((float(f32(p[k])) - self.gmin[k]) / self.res)
            out.append(min(max(v, 0), self.dims[k] - 1))
        return tuple(out)

    def _occupied(self, p, nearest, key0, res):
        """updateGridMap (:102-140): L-infinity distance to the closest point of the nearest occupied CELL < radius - 1e-5.  Without a cell
        within max_dist (or outside the distance map) closest_point stays default-constructed: a cell at the world origin."""
        idx = [int(math.floor((1.0 / res) * float(p[k]))) - int(key0[k]) for k in range(3)]
        dims = nearest.shape[::-1]
        code = 0
        if all(0 <= idx[k] < dims[k] for k in range(3)):
            code = int(nearest[idx[2], idx[1], idx[0]])
        if code >> 24:
            off = [(code & 255) - 128, ((code >> 8) & 255) - 128, ((code >> 16) & 255) - 128]
            c = [f32((idx[k] + off[k] + int(key0[k]) + 0.5) * res) for k in range(3)]
        else:
            c = [f32(0.0)] * 3
        delta = f32(0.5 * res)
        dist = 0.0
        for k in range(3):
            lo, hi = f32(c[k] - delta), f32(c[k] + delta)
            q = lo if p[k] < lo else (hi if p[k] > hi else p[k])
            dist = max(dist, abs(float(f32(q - p[k]))))
        return dist < self.radius - EPS_FLOAT

    def clear(self, points):
        """updateGridMission (:255-283), for every agent of the mission at once (difference 1)."""
        self.free = ~self.occ
        for p in points:
            i, j = self.node(p)
            self.free[j, i] = True

    NB = ((-1, 0), (1, 0), (0, -1), (0, 1))  # Grid::Grid: left, right, up (y - 1), down (y + 1)

    def neighbours(self, n):
        out = []
        for d in self.NB:
            m = (n[0] + d[0], n[1] + d[1])
            if 0 <= m[0] < self.W and 0 <= m[1] < self.H and self.free[m[1], m[0]]:
                out.append(m)
        return out

    def field(self, goal_node):
        """createDistanceTable: BFS from the goal node; field[y, x]."""
        D = np.full((self.H, self.W), UNREACHABLE, np.int64)
        D[goal_node[1], goal_node[0]] = 0
        q = collections.deque([goal_node])
        while q:
            n = q.popleft()
            d = D[n[1], n[0]]
            for m in self.neighbours(n):
                if d + 1 >= D[m[1], m[0]]:
                    continue
                D[m[1], m[0]] = d + 1
                q.append(m)
        return D


def mission_fields(grid, starts, goals):
    """(fields (n, H, W), init_d (n,)) after clearing the start and goal nodes of the mission."""
    grid.clear(list(starts) + list(goals))
    cache = {}
    F = []
    for g in goals:
        gn = grid.node(g)
        if gn not in cache:
            cache[gn] = grid.field(gn)
        F.append(cache[gn])
    init_d = [int(F[i][grid.node(s)[1], grid.node(s)[0]]) for i, s in enumerate(starts)]
    return np.array(F), np.array(init_d)


def linf(a, b):  # LInfinityDistance of two point3d (include/util.hpp:122-131)
    return max(abs(float(f32(f32(a[k]) - f32(b[k])))) for k in range(3))


def norm(a, b):  # (a - b).norm() of octomath::Vector3: float differences and sum, sqrt in double
    s = f32(0)
    for k in range(3):
        e = f32(f32(a[k]) - f32(b[k]))
        s = f32(s + f32(e * e))
    return math.sqrt(float(s))


def linf_to(p, Q):  # linf(p, q) for every row q of Q, the same float32 arithmetic element by element
    return np.abs((f32(p)[None, :] - Q.astype(f32)).astype(f32)).astype(np.float64).max(axis=1)


def norm_to(p, Q):  # norm(p, q) for every row q of Q
    e = (np.asarray(p, dtype=f32)[None, :] - Q.astype(f32)).astype(f32)
    s = f32(0) + (e[:, 0] * e[:, 0]).astype(f32)
    s = (s + (e[:, 1] * e[:, 1]).astype(f32)).astype(f32)
    s = (s + (e[:, 2] * e[:, 2]).astype(f32)).astype(f32)
    return np.sqrt(s.astype(np.float64))


def groups_of(positions, rng):
    """decentralizedMAPP :162-193, as the reference has it (ordered sets, merged the way it merges them); the walk over a group's
    members looking for one in range is a vector expression."""
    P = np.asarray(positions, dtype=np.float64).astype(f32)
    n = len(P)
    groups = [{0}]
    for qi in range(1, n):
        cand = -1
        gi = 0
        while gi < len(groups):
            members = sorted(groups[gi])
            if rng < 0 or (linf_to(P[qi], P[members]) < rng).any():
                if cand == -1:
                    groups[gi].add(qi)
                    cand = gi
                else:
                    groups[cand] |= groups[gi]
                    del groups[gi]
                    gi -= 1
            gi += 1
        if cand == -1:
            groups.append({qi})
    return [sorted(g) for g in groups]


def pibt_step(grid, cur, fields, init_d, ids):
    """One timestep of PIBT::run for the agents `ids` (a group, ascending): cur[i] node, fields[i], init_d[i] indexed by agent id.
    Returns {id: next node}.  chooseNode's candidates in the identity order (difference 2).  An agent's own node is a node of its graph
    (the stay candidate) whatever the map says; occupied nodes are nobody's neighbours."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * len(ids) + 1000))
    n = len(ids)
    now, nxt, vnext = {}, {}, {i: None for i in ids}
    for i in ids:
        now[cur[i]] = i  # occupied_now[s->id] = a: a later agent overwrites
    # priority queue: elapsed (0), init_d, tie_breaker = index / n -- the top is the LARGEST
    order = sorted(ids, key=lambda i: (init_d[i], f32(ids.index(i)) / f32(n)), reverse=True)

    def dist(i, u):
        return int(fields[i][u[1], u[0]])

    def choose(a):
        C = grid.neighbours(cur[a]) + [cur[a]]
        v = None
        for u in C:
            if u in nxt:
                continue
            j = now.get(u)
            if j is not None and vnext[j] == cur[a]:
                continue
            if dist(a, u) == 0:  # u == a->g
                return u
            if v is None:
                v = u
            else:
                cv, cu = dist(a, v), dist(a, u)
                if cu < cv or (cu == cv and v in now and u not in now):
                    v = u
        return v

    def plan_one_step(a):
        v = choose(a)
        if v is not None:
            nxt[v] = a
            vnext[a] = v
        return v

    def func_pibt(ai):
        v = plan_one_step(ai)
        while v is not None:
            aj = now.get(v)
            if aj is not None:
                if aj != ai and vnext[aj] is None:
                    if not func_pibt(aj):
                        v = plan_one_step(ai)
                        continue
            return True
        nxt[cur[ai]] = ai
        vnext[ai] = cur[ai]
        return False

    for a in order:
        if vnext[a] is None:
            func_pibt(a)
    return vnext


def waypoint_step(grid, rng, positions, plans_pts, current_goals, waypoints, fields, init_d, use_filter=True):
    """One decentralizedMAPP for the whole mission.
    positions (n, 3), plans_pts: per agent the M + 1 points the filter looks at (segment start points, then the last point) or None
    (no trajectory yet), current_goals (n, 3), waypoints (n, 3).
    Returns (group label = least id (n,), desired node (n,) as y * W + x, updated (n,), new waypoints (n, 3))."""
    n = len(waypoints)
    way = np.array(waypoints, dtype=np.float64).copy()
    label, desired, updated = np.zeros(n, int), np.zeros(n, int), np.zeros(n, int)
    cur = [grid.node(way[i]) for i in range(n)]
    for group in groups_of(positions, rng):
        for i in group:
            label[i] = group[0]
        vnext = pibt_step(grid, cur, fields, init_d, group)
        des_pt = {i: grid.point(vnext[i]) for i in group}
        for i in group:
            desired[i] = vnext[i][1] * grid.W + vnext[i][0]
        if not use_filter:
            for i in group:
                way[i] = des_pt[i]
                updated[i] = 1
            continue
        cand = set()
        for qi in group:
            in_range = True
            if rng > 0:
                pts = plans_pts[qi] if plans_pts is not None and plans_pts[qi] is not None else [positions[qi]]
                for p in pts:
                    if linf(des_pt[qi], p) > 0.5 * rng - EPS_FLOAT:
                        in_range = False
                        break
            if in_range and norm(des_pt[qi], way[qi]) > EPS_FLOAT and norm(current_goals[qi], way[qi]) < EPS_FLOAT:
                cand.add(qi)
        # "find valid update" (:266-296), the loop as the reference has it
        update = False
        garr = np.array(group)
        D = np.array([des_pt[i] for i in group], dtype=f32)
        while not update and cand and len(group) > 1:
            for qi in sorted(cand):
                # for qj in group (qj != qi): next_waypoint_j = waypoint of a non-candidate, desired waypoint of a candidate; the first
                # one within 1e-5 of qi's desired waypoint drops qi and restarts -- "any" of a vector expression
                is_c = np.array([j in cand for j in group])
                nw = np.where(is_c[:, None], D, way[garr].astype(f32))
                occupied = (norm_to(des_pt[qi], nw) < EPS_FLOAT) & (garr != qi)
                if occupied.any():
                    cand.discard(qi)
                    update = False
                    break
                update = True
        for qi in cand:
            way[qi] = des_pt[qi]
            updated[qi] = 1
    return label, desired, updated, way
