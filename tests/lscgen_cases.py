"""Constructed inputs for the LSC generators (csrc/lscgen.hip) that state their result by construction -- TEST INFRASTRUCTURE.

A case is one six-point hull of relative control points, given in the frame the generators work in (z already divided by the pair's
downwash).  Every coordinate is a small integer times a power of two, so the float32 staging of the generators is exact on both
sides and the only arithmetic under test is the closest-point search and what follows it.

Recipe of a `hull` case: an integer normal nv of integer length nl, integer in-plane vectors u, v (both orthogonal to nv), the foot at
c nv; the winning feature's one, two or three points lie on the plane nv . x = c nl^2 around the foot, every other point strictly
beyond it.  The closest point is then the foot, the unit normal nv / nl, and d_i = (r_a + r_b + rel_i . n) / 2 follows.

kinds:  "hull"    the origin is outside, farther than 1e-5: the hull's normal
        "near"    outside but closer than 1e-5 (float32): generateLSC falls back, generateCLSC keeps the hull's normal
        "inside"  the origin is in the hull: generateLSC falls back to goal - obstacle position, generateCLSC writes a zero normal
"""
from itertools import combinations

import numpy as np

# (nv, nl, u, v): u . nv = v . nv = 0, u and v independent
FRAMES_3D = [((1, 2, 2), 3, (2, -1, 0), (2, 0, -1)), ((2, 3, 6), 7, (3, -2, 0), (0, 2, -1)), ((0, 0, 1), 1, (1, 0, 0), (0, 1, 0)),
             ((-3, 0, 4), 5, (4, 0, 3), (0, 1, 0)), ((-2, -1, 2), 3, (1, -2, 0), (1, 0, 1)), ((6, -2, 3), 7, (1, 3, 0), (0, 3, 2)),
             ((0, -1, 0), 1, (1, 0, 0), (0, 0, 1)), ((2, -2, -1), 3, (1, 1, 0), (1, 0, 2))]
FRAMES_2D = [((3, 4, 0), 5, (4, -3, 0)), ((0, 1, 0), 1, (1, 0, 0)), ((-5, 12, 0), 13, (12, 5, 0)), ((-4, -3, 0), 5, (3, -4, 0)),
             ((-1, 0, 0), 1, (0, 1, 0))]
FEATURES_3D = [S for k in (1, 2, 3) for S in combinations(range(6), k)]  # 6 + 15 + 20 = 41, the kernel's enumeration order
FEATURES_2D = [S for k in (1, 2) for S in combinations(range(6), k)]     # 6 + 15 = 21
FALLBACKS = [(2, 3, 6), (1, 2, 2), (-3, 0, 4), (0, 0, -1), (4, -3, 0), (6, -2, 3), (-2, -6, 3)]  # integer vectors of integer length


def _v(x):
    return np.array(x, dtype=np.float64)


def case(name, family, rel, kind="hull", n=None, winner=None, dim=3, dwk=1, obs_max=8.0, obs_step=0.25, fb=None):
    """n: the expected unit normal in the transformed frame (None: ask the referee); winner: the subset that must win (None: ties);
    dwk: the pair's downwash (1 or 2); obs_*: range / granularity of the neighbour's own trajectory; fb = "zero": goal == obstacle."""
    return dict(name=name, family=family, rel=_v(rel), kind=kind, n=None if n is None else _v(n), winner=winner, dim=dim, dwk=dwk,
                obs_max=obs_max, obs_step=obs_step, fb=fb)


def _beyond(foot, nv, u, v, j):
    """the j-th point strictly beyond the supporting plane through the foot (distinct for distinct j)"""
    return foot + nv * (j + 1) / 4 + u * ((j % 3) - 1) / 2 + v * (((j + 1) % 3) - 1) / 2


def feature_hull(S, frame, c, dim=3):
    nv, nl, u = _v(frame[0]), frame[1], _v(frame[2])
    v = _v(frame[3]) if dim == 3 else np.zeros(3)
    foot = c * nv
    on = {1: [foot], 2: [foot - u / 4, foot + u / 2], 3: [foot - u / 4 - v / 4, foot + u / 2, foot + v / 2]}[len(S)]
    pts = np.zeros((6, 3))
    j = 0
    for i in range(6):
        if i in S:
            pts[i] = on[S.index(i)]
        else:
            pts[i] = _beyond(foot, nv, u, v, j)
            j += 1
    return pts, nv / nl


def feature_cases(dim, dwk, frames, scales=(0.25, 0.5, 1.0, 0.75)):
    """every feature the unique winner, once per frame"""
    out = []
    for S in (FEATURES_3D if dim == 3 else FEATURES_2D):
        for q, fr in enumerate(frames):
            pts, n = feature_hull(S, fr, scales[(q + len(S)) % len(scales)], dim)
            out.append(case("feature%s/%s/dw%d" % (S, fr[0], dwk), "feature%dd" % dim, pts, n=n, winner=S, dim=dim, dwk=dwk))
    return out


def degenerate_cases():
    out = []
    for q, fr in enumerate((FRAMES_3D[0], FRAMES_3D[1], FRAMES_3D[3], FRAMES_3D[6])):
        nv, nl, u, v = _v(fr[0]), fr[1], _v(fr[2]), _v(fr[3])
        n = nv / nl
        foot = (0.5, 0.25, 1.0, 0.75)[q] * nv
        tag = "/%s" % (fr[0],)
        add = lambda name, pts, **kw: out.append(case(name + tag, "degenerate", pts, **kw))  # noqa: E731
        # all six points equal: the last segment of every shifted plan
        add("all-equal", [foot] * 6, n=n, winner=(0,))
        b = [_beyond(foot, nv, u, v, j) for j in range(5)]
        # repeated points: the winning vertex twice; both ends of the winning edge twice; losers twice
        add("vertex-twice", [foot, b[0], b[1], foot, b[2], b[3]], n=n, winner=(0,))
        A, B = foot - u / 4, foot + u / 2
        add("edge-ends-twice", [A, B, A, b[0], B, b[1]], n=n, winner=(0, 1))
        add("losers-twice", [b[0], b[0], foot, b[1], b[1], b[2]], n=n, winner=(2,))
        # collinear hulls (every triangle is degenerate): closest point inside an edge, then at an end
        add("collinear-interior", [foot + u * t for t in (-0.25, 0.5, 1.0, -1.0, 2.0, -2.0)], n=n)
        add("collinear-end", [foot + (u + nv) * t for t in (0.5, 0.25, 1.0, 0.0, 2.0, 1.5)], n=n, winner=(3,))
        # coplanar hulls in a 3-D mission: foot inside the polygon (triangles tie); plane through the origin with the origin outside
        # (an edge wins); origin inside the polygon (fallback)
        add("coplanar-foot-inside", [foot + w for w in (u / 2, v / 2, -(u + v) / 2, (2 * u + v) / 4, (2 * v - u) / 4, -(u + 3 * v) / 4)], n=n)
        add("plane-through-origin-edge", [b_ if i not in (1, 4) else (A if i == 1 else B)
                                          for i, b_ in enumerate([foot + nv * (j + 1) / 4 + u * ((j % 3) - 1) / 2 for j in range(6)])],
            n=n, winner=(1, 4))
        add("plane-through-origin-inside", [nv, -nv, u, -u, (nv + u) / 2, -(nv + u) / 2], kind="inside")
        add("plane-through-origin-inside-triangle", [nv, u, -(nv + u), nv / 2, u / 2, (nv + u) / 4], kind="inside")
    return out


def sliver_cases():
    """triangles of height 2^-10 and 2^-20 of their base: held to the referee (n=None), not to a constructed answer"""
    out = []
    for fr, c in ((FRAMES_3D[2], 0.5), (FRAMES_3D[6], 1.0), (FRAMES_3D[0], 0.25)):
        nv, u, v = _v(fr[0]), _v(fr[2]), _v(fr[3])
        foot = c * nv
        for e in (10, 20):
            h = 2.0 ** -e
            for skew, S in ((0.0, (0, 1, 2)), (0.25, (1, 3, 5))):
                on = [foot - u / 2 - v * h / 2, foot + u / 2 - v * h / 2, foot + v * h / 2 + u * skew]
                pts, j = np.zeros((6, 3)), 0
                for i in range(6):
                    if i in S:
                        pts[i] = on[S.index(i)]
                    else:
                        pts[i] = _beyond(foot, nv, u, v, j)
                        j += 1
                out.append(case("sliver-2^-%d/%s/skew%g" % (e, fr[0], skew), "sliver", pts, winner=S, obs_max=1.0))
    return out


def switch_cases():
    """the float32 threshold len < 1e-5f: closest vertex at 2^-17 m (fallback) and at 2^-16 m (the hull's normal)"""
    out = []
    for e, kind in ((17, "near"), (16, "hull")):
        s = 2.0 ** -e
        for fr in (FRAMES_3D[2], FRAMES_3D[6], ((-1, 0, 0), 1, (0, 1, 0), (0, 0, 1))):  # on an axis: exact
            nv, u, v = _v(fr[0]), _v(fr[2]), _v(fr[3])
            foot = s * nv
            pts = [_beyond(foot, nv, u, v, j) for j in range(5)]
            pts.insert(4, foot)
            out.append(case("switch-2^-%d/%s" % (e, fr[0]), "switch", pts, kind=kind, n=nv, winner=(4,), obs_max=2.0))
        # on (1,2,2)/3: the vertex is the float32 rounding of (s/3)(1,2,2); the referee states the normal
        nv, u, v = _v((1, 2, 2)), _v((2, -1, 0)), _v((2, 0, -1))
        foot = np.float32(s / 3 * nv).astype(np.float64)
        pts = [nv * (j + 1) / 4 + u * ((j % 3) - 1) / 2 + v * (((j + 1) % 3) - 1) / 2 for j in range(5)]
        pts.insert(2, foot)
        out.append(case("switch-2^-%d/(1,2,2)" % e, "switch", pts, kind=kind, winner=(2,), obs_max=0.0))
    return out


def inside_cases():
    """a tetrahedron plus two points, the origin 2^-10 m outside one face (that face's normal) and 2^-10 m inside it (fallback)"""
    out = []
    for q, (fr, eps) in enumerate(((FRAMES_3D[2], 2.0 ** -10), (((0, 0, -1), 1, (1, 0, 0), (0, 1, 0)), 2.0 ** -10), (((1, 0, 0), 1, (0, 1, 0), (0, 0, 1)), 2.0 ** -10),
                                   (FRAMES_3D[6], 2.0 ** -10), (FRAMES_3D[0], 2.0 ** -12))):  # ((1,2,2): 3 * 2^-12 m)
        nv, nl, u, v = _v(fr[0]), fr[1], _v(fr[2]), _v(fr[3])
        S = ((0, 1, 2), (3, 4, 5), (0, 2, 5), (1, 3, 4), (2, 3, 5))[q]
        for side, kind in ((+1, "hull"), (-1, "inside")):
            foot = side * eps * nv
            on = [foot - u / 4 - v / 4, foot + u / 2, foot + v / 2]
            far = [foot + nv, foot + nv * 1.25 + u / 4, foot + nv * 1.5 - v / 4]
            pts, j = np.zeros((6, 3)), 0
            for i in range(6):
                if i in S:
                    pts[i] = on[S.index(i)]
                else:
                    pts[i] = far[j]
                    j += 1
            out.append(case("face-%s/%s" % ("outside" if side > 0 else "inside", fr[0]), "inside", pts, kind=kind,
                            n=nv / nl if side > 0 else None, winner=S if side > 0 else None, obs_max=2.0))
    return out


def inside_cases_2d():
    pts = [(1, 0, 0), (0, 1, 0), (-1, -1, 0), (0.5, 0.5, 0), (-0.5, 0, 0), (0, -0.5, 0)]
    out = [case("polygon-around-origin", "inside", pts, kind="inside", dim=2),
           case("polygon-around-origin-shifted", "inside", _v(pts) + _v((0.125, -0.25, 0)), kind="inside", dim=2)]
    out += [case("all-equal-2d", "degenerate", [_v((3, 4, 0)) / 4] * 6, n=_v((3, 4, 0)) / 5, winner=(0,), dim=2)]
    return out


def zero_goal_cases(dim):
    """goal == obstacle position on an overlapping pair: zero normal, b = (r_a + r_b) / 2, everything finite"""
    pts = [(1, 0, 0), (0, 1, 0), (-1, -1, 0), (0.5, 0.5, 0.5 if dim == 3 else 0), (-0.5, 0, -1 if dim == 3 else 0), (0, -0.5, 0)]
    return [case("goal-on-obstacle-%d" % q, "fallback", _v(pts) * s, kind="inside", dim=dim, fb="zero") for q, s in enumerate((1.0, 0.5, 2.0))] + \
           [case("goal-on-obstacle-coincident", "fallback", np.zeros((6, 3)), kind="inside", dim=dim, fb="zero")]


def all_cases_3d():
    return (feature_cases(3, 1, FRAMES_3D[:4]) + feature_cases(3, 2, FRAMES_3D[4:8]) + degenerate_cases() + sliver_cases() + switch_cases()
            + inside_cases() + zero_goal_cases(3))


def all_cases_2d():
    return feature_cases(2, 1, FRAMES_2D[:4]) + inside_cases_2d() + zero_goal_cases(2)


# ---- what the generators must write for a case --------------------------------------------------------------------------------
def referee_normal(c, referee):
    """(kind, unit normal or None) of a hull from the exact referee: the 1e-5f rule applied to the float32 closest point"""
    r = referee.closest_point(c["rel"])
    if r.inside:
        return "inside", None, r
    cf = np.array([float(x) for x in r.point]).astype(np.float32)
    length = np.sqrt(np.float32(cf[0] * cf[0] + cf[1] * cf[1] + cf[2] * cf[2]))
    return ("near" if length < np.float32(1e-5) else "hull"), np.array(referee.unit_normal(r)), r


def expected_rows(c, n_t, p_obs, margin_sum, dw, fb, mode, dim, fixed_margin=None):
    """Rows (nx, ny, nz, b)[6] of one unit.  n_t: the hull's unit normal in the transformed frame (used for kind "hull", and for "near" in
    CLSC); p_obs (6, 3): the obstacle's points; fb: goal - obstacle position; mode "lsc" | "clsc" | "obstacle"; fixed_margin: d of
    the obstacle generator (predicted size + agent radius) instead of (r_a + r_b + rel . n) / 2."""
    use_hull = c["kind"] == "hull" or (c["kind"] == "near" and mode == "clsc")
    if use_hull:
        n = np.array(n_t, dtype=np.float64)
    elif mode == "clsc":
        n = np.zeros(3)
    else:
        f = np.array([fb[0], fb[1], fb[2] / dw if dim == 3 else 0.0])
        ln = np.linalg.norm(f)
        n = f / ln if ln > 0 else np.zeros(3)
    rel = c["rel"].copy()
    if dim == 2 and mode != "clsc":
        rel[:, 2] = 0.0
    d = 0.5 * (margin_sum + rel @ n) if fixed_margin is None else np.full(6, fixed_margin)
    n_out = np.array([n[0], n[1], n[2] / dw if (dim == 3 or mode == "clsc") else 0.0])
    out = np.zeros((6, 4))
    out[:, :3] = n_out
    out[:, 3] = d + p_obs @ n_out
    return out


PAIRS = {1: [(0.15, 0.15, 1.0, 1.0), (0.25, 0.75, 1.0, 1.0)],                               # (r_a, r_b, dw_a, dw_b) -> downwash 1
         2: [(0.15, 0.15, 2.0, 2.0), (0.25, 0.75, 5.0, 1.0), (0.25, 0.5, 2.0, 2.0)]}       # -> exactly 2 (radius weighted: 1.25 + 0.75)


def _exact32(a):
    return np.array_equal(np.float32(a).astype(np.float64), a)


def pack_pairs(cases, M, dim, hull_segments=None, seed=0, z_noise=False):
    """One hull per (agent, segment), n_obs = 1, the partner of agent a appended behind the planning agents as agent N + a.
    hull_segments < M (generateCLSC: the last segment is not a hull): the cases fill the first hull_segments segments only.
    Returns the launch inputs and slot[a][m] = index of the case in (a, m) (or -1)."""
    hs = M if hull_segments is None else hull_segments
    rng = np.random.default_rng(seed)
    order = sorted(range(len(cases)), key=lambda i: (cases[i]["dwk"], cases[i]["fb"] == "zero", cases[i]["obs_max"]))
    groups, cur = [], []
    for i in order:
        key = (cases[i]["dwk"], cases[i]["fb"])
        if cur and (len(cur) == hs or (cases[cur[0]]["dwk"], cases[cur[0]]["fb"]) != key):
            groups.append(cur)
            cur = []
        cur.append(i)
    groups.append(cur)
    N = len(groups)
    traj = np.zeros((2 * N, M, 6, 3))
    radius, downwash = np.zeros(2 * N), np.zeros(2 * N)
    goal = np.zeros((2 * N, 3))
    slot = -np.ones((N, M), dtype=np.int64)
    fbs, dws = np.zeros((N, 3)), np.zeros(N)
    for a, g in enumerate(groups):
        dwk = cases[g[0]]["dwk"] if dim == 3 else 1
        ra, rb, da, db = PAIRS[dwk][a % len(PAIRS[dwk])]
        radius[a], radius[N + a], downwash[a], downwash[N + a] = ra, rb, da, db
        dws[a] = dwk
        for m in range(M):
            ci = g[m] if m < len(g) else g[0]
            c = cases[ci]
            if m < len(g):
                slot[a, m] = ci
            step, top = c["obs_step"], c["obs_max"]
            k = int(top / step)
            p = rng.integers(-k, k + 1, (6, 3)) * step if k > 0 else np.zeros((6, 3))
            rel = c["rel"].copy()
            if dim == 2:
                p[:, 2] = 1.0
                rel[:, 2] = rng.integers(-8, 9, 6) * 0.25 if z_noise else 0.0  # z is ignored by generateLSC in 2-D: z_2d arbitrary
            own = p + rel * np.array([1.0, 1.0, float(dwk)])
            traj[a, m], traj[N + a, m] = own, p
            # float32 staging is exact: the inputs are float32 values and the generators' float32 difference reproduces rel
            assert _exact32(own) and _exact32(p), c["name"]
            d32 = (np.float32(own) - np.float32(p)).astype(np.float64)
            assert np.array_equal(d32[:, :2], c["rel"][:, :2]), c["name"]
            if dim == 3:
                dz = (np.float32(own[:, 2]) / np.float32(dwk) - np.float32(p[:, 2]) / np.float32(dwk)).astype(np.float64)
                assert np.array_equal(dz, c["rel"][:, 2]), c["name"]
        fb = np.zeros(3) if cases[g[0]]["fb"] == "zero" else _v(FALLBACKS[a % len(FALLBACKS)]) * np.array([1.0, 1.0, float(dwk)])
        fbs[a] = fb
        goal[a] = traj[N + a, 0, 0] + fb  # the fallback uses the FIRST control point of the neighbour's plan, for every segment
        goal[N + a] = traj[N + a, M - 1, 5] + np.array([0.5, -0.25, 0.0])
    if dim == 2 and not z_noise:
        goal[:, 2] = 1.0  # a 2-D mission proper: every z is z_2d (generateCLSC does not drop z, it relies on this)
    nbr = (N + np.arange(N, dtype=np.int32)).reshape(N, 1)
    return dict(N=N, traj=traj, nbr=nbr, radius=radius, downwash=downwash, goal_all=goal, slot=slot, fb=fbs, dw=dws, M=M, dim=dim)


def expected_for_pack(cases, pk, normals, mode):
    """(N, M, 6, 4) expected rows of pack_pairs' launch (NaN where no case sits, e.g. generateCLSC's last segment)"""
    N, M = pk["N"], pk["M"]
    want = np.full((N, M, 6, 4), np.nan)
    for a in range(N):
        for m in range(M):
            ci = pk["slot"][a, m]
            if ci < 0:
                continue
            want[a, m] = expected_rows(cases[ci], normals[ci], pk["traj"][N + a, m], pk["radius"][a] + pk["radius"][N + a], pk["dw"][a],
                                       pk["fb"][a], mode, pk["dim"])
    return want


OBSTACLE_PAIRS = {1: [(0.15, 0.35, 1.0), (0.25, 0.75, 1.0)], 2: [(0.5, 0.5, 3.0), (0.75, 0.25, 5.0)]}  # (r_own, radius, downwash) -> 1, 2
TALL = (0.25, 0.25, 4.0, 2.5)  # a type-0 obstacle above obs_downwash_threshold = 3: planar separation; downwashBetween = 1.25 / 0.5


def pack_obstacles(cases, M, dim, tall=False, seed=0):
    """One static obstacle per agent (velocity 0: its six predicted points are its position), one hull per (agent, segment)."""
    rng = np.random.default_rng(seed)
    order = sorted(range(len(cases)), key=lambda i: (cases[i]["dwk"], cases[i]["fb"] == "zero", cases[i]["obs_max"]))
    groups, cur = [], []
    for i in order:
        key = (cases[i]["dwk"], cases[i]["fb"])
        if cur and (len(cur) == M or (cases[cur[0]]["dwk"], cases[cur[0]]["fb"]) != key):
            groups.append(cur)
            cur = []
        cur.append(i)
    groups.append(cur)
    N = len(groups)
    traj, radius, goal = np.zeros((N, M, 6, 3)), np.zeros(N), np.zeros((N, 3))
    table = np.zeros(N, dtype=[("position", "f8", 3), ("velocity", "f8", 3), ("radius", "f8"), ("downwash", "f8"), ("max_acc", "f8"),
                               ("type", "i4"), ("reserved", "i4")])
    slot = -np.ones((N, M), dtype=np.int64)
    fbs, dws = np.zeros((N, 3)), np.zeros(N)
    for a, g in enumerate(groups):
        dwk = cases[g[0]]["dwk"] if dim == 3 else 1
        if tall:
            r_own, r_ob, dw_ob, dw = TALL
            typ = 0
        else:
            r_own, r_ob, dw_ob = OBSTACLE_PAIRS[dwk][a % 2]
            dw, typ = float(dwk), 1
        if dim == 2:
            dw = 1.0
        top = min(cases[i]["obs_max"] for i in g)
        k = int(top / 0.25)
        pos = rng.integers(-k, k + 1, 3) * 0.25 if k > 0 else np.zeros(3)
        if dim == 2:
            pos[2] = 1.0
        radius[a] = r_own
        table[a]["position"], table[a]["radius"], table[a]["downwash"], table[a]["max_acc"], table[a]["type"] = pos, r_ob, dw_ob, 1.5, typ
        dws[a] = dw
        for m in range(M):
            ci = g[m] if m < len(g) else g[0]
            if m < len(g):
                slot[a, m] = ci
            rel = cases[ci]["rel"].copy()
            if tall or dim == 2:
                rel[:, 2] = rng.integers(-8, 9, 6) * 0.25  # dropped by the generator
            own = pos + rel * np.array([1.0, 1.0, dw if not tall else 1.0])
            traj[a, m] = own
            assert _exact32(own), cases[ci]["name"]
            d32 = (np.float32(own) - np.float32(pos)).astype(np.float64)
            assert np.array_equal(d32[:, :2], cases[ci]["rel"][:, :2]), cases[ci]["name"]
            if dim == 3 and not tall:
                dz = (np.float32(own[:, 2]) / np.float32(dw) - np.float32(pos[2]) / np.float32(dw)).astype(np.float64)
                assert np.array_equal(dz, cases[ci]["rel"][:, 2]), cases[ci]["name"]
        fb = np.zeros(3) if cases[g[0]]["fb"] == "zero" else _v(FALLBACKS[a % len(FALLBACKS)]) * np.array([1.0, 1.0, dw])
        fbs[a] = fb
        goal[a] = pos + fb
    return dict(N=N, traj=traj, radius=radius, goal=goal, table=table, ids=np.arange(N, dtype=np.int32).reshape(N, 1), slot=slot, fb=fbs,
                dw=dws, M=M, dim=dim, tall=tall)


def expected_for_obstacles(cases, pk, normals):
    N, M = pk["N"], pk["M"]
    want = np.full((N, M, 6, 4), np.nan)
    for a in range(N):
        for m in range(M):
            ci = pk["slot"][a, m]
            if ci < 0:
                continue
            c = cases[ci]
            if pk["tall"] or pk["dim"] == 2:
                c = dict(c, rel=c["rel"] * np.array([1.0, 1.0, 0.0]))
            pos = np.tile(pk["table"][a]["position"], (6, 1))
            want[a, m] = expected_rows(c, normals[ci], pos, 0.0, pk["dw"][a], pk["fb"][a], "obstacle", pk["dim"],
                                       fixed_margin=pk["table"][a]["radius"] + pk["radius"][a])
    return want


# ---- the suites, built once per session and shared by the CPU and the GPU tests -----------------------------------------------
_CACHE = {}


def suite(dim):
    """(cases, kinds, referee normals, constructed-or-referee normals) of every constructed family of one dimension"""
    if dim not in _CACHE:
        from tests import hull_reference as R

        cases = all_cases_3d() if dim == 3 else all_cases_2d()
        ref = []
        for c in cases:
            hull = c["rel"] * np.array([1.0, 1.0, 1.0 if dim == 3 else 0.0])
            ref.append(referee_normal(dict(c, rel=hull), R))
        n_ref = [r[1] for r in ref]
        n_con = [c["n"] if c["n"] is not None else r[1] for c, r in zip(cases, ref)]
        _CACHE[dim] = (cases, ref, n_ref, n_con)
    return _CACHE[dim]


def golden_hulls():
    """The recorded openGJK hulls (tests/golden/gjk_hulls.json: 240, gjk_hulls_3000.npz: 3000) rounded to float32, with the recorded
    distances; `planar`: those whose un-rounded points lie in one plane (their xy projections serve the 2-D generators)."""
    if "golden" not in _CACHE:
        import os

        from tests import helpers as H

        g = H.load_golden("gjk_hulls")
        z = np.load(os.path.join(H.GOLDEN, "gjk_hulls_3000.npz"))
        raw = np.concatenate([np.array([c["hull"] for c in g["cases"]], dtype=np.float64), z["hull"]])
        dist = np.concatenate([np.array([c["dist"] for c in g["cases"]]), z["dist"]])
        centred = raw - raw.mean(1, keepdims=True)
        planar = np.linalg.svd(centred, compute_uv=False)[:, 2] <= 1e-9 * np.abs(raw).max((1, 2))
        _CACHE["golden"] = (np.float32(raw).astype(np.float64), dist, planar)
    return _CACHE["golden"]


def golden_suite(dim):
    """the golden hulls as cases (dim 3: all 3240; dim 2: the xy projections of the planar ones), kind and normal from the referee"""
    key = ("golden", dim)
    if key not in _CACHE:
        from tests import hull_reference as R

        hulls, _, planar = golden_hulls()
        if dim == 2:
            hulls = hulls[planar] * np.array([1.0, 1.0, 0.0])
        cases = [case("golden%d" % i, "golden%dd" % dim, h, kind="?", dim=dim, obs_max=0.0) for i, h in enumerate(hulls)]
        ref = [referee_normal(c, R) for c in cases]
        for c, r in zip(cases, ref):
            c["kind"] = r[0]
        n_ref = [r[1] for r in ref]
        _CACHE[key] = (cases, ref, n_ref, n_ref)
    return _CACHE[key]


# ---- device runners ------------------------------------------------------------------------------------------------------------
def rows_array(buf, api, rows_f32, shape):
    r = buf.view(api.ROW_F32_DTYPE if rows_f32 else api.ROW_DTYPE).reshape(shape)
    return np.stack([r["nx"], r["ny"], r["nz"], r["b"]], axis=-1).astype(np.float64)


def run_pairs_device(api, mode, pk, entry="constraints", rows_f32=False):
    """pack_pairs' launch through generate_lsc_device (entry "lsc") or generate_constraints_device: (N, M, 6, 4) rows"""
    import torch

    dev = torch.device("cuda", 0)
    kw = dict(row_format=api.ROWS_F32) if rows_f32 else {}
    sol = api.Solver(api.make_desc(M=pk["M"], dim=pk["dim"], world_min=(-40, -40, -40), world_max=(40, 40, 40), **kw))
    N, M = pk["N"], pk["M"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    item = 16 if rows_f32 else 32
    d_rows = torch.full((N * M * 6 * item,), 0xFF, dtype=torch.uint8, device=dev)
    args = (N, 1, 0, up(pk["traj"]), up(pk["nbr"]), up(pk["radius"]), up(pk["downwash"]))
    if entry == "lsc":
        sol.generate_lsc_device(*args, up(pk["goal_all"][:N]), d_rows)
    else:
        sol.generate_constraints_device(mode, *args, up(pk["goal_all"]), d_rows)
    torch.cuda.synchronize()
    return rows_array(d_rows.cpu().numpy(), api, rows_f32, (N, M, 6))


def oracle_pairs(oracle, api, mode, pk):
    L = oracle.generate_constraints(mode, pk["traj"], pk["nbr"], pk["radius"], pk["downwash"], pk["goal_all"], dim=pk["dim"])
    r = api.pack_rows(L).reshape(pk["N"], pk["M"], 6)
    return np.stack([r["nx"], r["ny"], r["nz"], r["b"]], axis=-1)


def obstacle_param(api):
    return api.ObstacleParam(1.0, 0.75, 3.0, 0.1, 0, 0)  # size prediction and velocity guard off: d = radius + r_own


def run_obstacles_device(api, pk, rows_f32=False):
    import torch

    dev = torch.device("cuda", 0)
    kw = dict(row_format=api.ROWS_F32) if rows_f32 else {}
    sol = api.Solver(api.make_desc(M=pk["M"], dim=pk["dim"], world_min=(-40, -40, -40), world_max=(40, 40, 40), **kw))
    N, M = pk["N"], pk["M"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    hdr = np.zeros(N, api.HEADER_DTYPE)
    hdr["amax"] = 2.0
    item = 16 if rows_f32 else 32
    d_rows = torch.full((N * M * 6 * item,), 0xFF, dtype=torch.uint8, device=dev)
    table = np.zeros(N, api.OBSTACLE_DTYPE)
    for f in ("position", "velocity", "radius", "downwash", "max_acc", "type"):
        table[f] = pk["table"][f]
    sol.generate_lsc_obstacles_device(obstacle_param(api), N, 1, 0, up(pk["traj"]), up(pk["ids"]), up(table), up(pk["radius"]), up(pk["goal"]),
                                      up(hdr), d_rows, 1, 0)
    torch.cuda.synchronize()
    return rows_array(d_rows.cpu().numpy(), api, rows_f32, (N, M, 6))


def oracle_obstacles(oracle, api, pk):
    op = oracle.obs_param(dt=0.2, obs_size_prediction=False, use_velocity_guard=False)
    out = np.zeros((pk["N"], pk["M"], 6, 4))
    for a in range(pk["N"]):
        ob = np.zeros((), oracle.OBSTACLE_DTYPE)
        for f in ("position", "velocity", "radius", "downwash", "max_acc", "type"):
            ob[f] = pk["table"][a][f]
        r = api.pack_rows(oracle.generate_lsc_obstacles(op, pk["traj"][a], pk["goal"][a], pk["radius"][a], np.zeros(3), 2.0, ob, dim=pk["dim"]))[0]
        out[a] = np.stack([r["nx"], r["ny"], r["nz"], r["b"]], axis=-1)
    return out
