"""An exact feasibility referee for the trajectory QP's row system, and the instance families that approach the solver's INFEASIBLE rules.

The referee judges the row-for-row model oracle.assemble() builds (G x <= h, Aeq x = beq, lb <= x <= ub) by

    t* = min over x with Aeq x = beq of  max_i (G_i x - h_i) / |G_i|        (metres; the variable bounds are rows too)

t* < 0: a point with margin -t* inside every row exists.  t* > 0: every point violates some row by t* or more.  One LP (HiGHS) finds a
candidate point and a dual; neither is trusted as it stands.  Both are re-evaluated in 50-digit arithmetic (mpmath):

  * t_hi: the LP's x, projected onto Aeq x = beq (iterative refinement in high precision), and its largest normalised row residual;
  * t_lo: weak duality.  For y >= 0 with sum y = 1 and any z, every x with Aeq x = beq has
        max_i r_i(x) >= sum_i y_i r_i(x) = -h~'y - beq'z + rho'x,    rho = G~'y + Aeq'z  (the dual's float residual),
    and rho'x is bounded below by the box the rows themselves imply (a variable pinned by the equality rows enters with its value; any
    other one lies within its bound rows widened by T, or the point violates a row by more than T anyway).

Labels: FEASIBLE if t_hi <= -1e-7, INFEASIBLE if t_lo >= 1e-5, GREY otherwise.  The 1e-5 bar leaves room for the kernels' own row scaling.

Families (ABI arrays in, ABI arrays out; generated, seeded):
  A  near-antiparallel pairs: one control point gets a second row whose normal is the first's, reversed and tilted by eps, overlapping by delta
     -- or a corridor face as the partner;
  B  graded slabs: bench.make_infeasible's mirror construction with a slab of width w instead of -0.4 m;
  C  empty and zero-width corridor intervals on one axis of one segment (and narrow open ones beside them).
"""
import math
from collections import Counter

import mpmath
import numpy as np

FEASIBLE, GREY, INFEASIBLE = "FEASIBLE", "GREY", "INFEASIBLE"
FEASIBLE_BAR, INFEASIBLE_BAR = -1e-7, 1e-5
_DPS = 50
_T_BOX = 1.0  # (m) the widening of the implied box in the dual bound


class Verdict:
    __slots__ = ("t_lo", "t_hi", "t_lp", "label")

    def __init__(self, t_lo, t_hi, t_lp):
        self.t_lo, self.t_hi, self.t_lp = t_lo, t_hi, t_lp
        self.label = FEASIBLE if t_hi <= FEASIBLE_BAR else INFEASIBLE if t_lo >= INFEASIBLE_BAR else GREY

    def __repr__(self):
        return "Verdict(%s, t_lo=%.6g, t_hi=%.6g)" % (self.label, self.t_lo, self.t_hi)


def _sparse_rows(A):
    idx = [np.flatnonzero(A[i]) for i in range(A.shape[0])]
    return idx, [A[i, ix] for i, ix in enumerate(idx)]


def judge(G, h, Aeq, beq, lb, ub):
    """Certified bounds t_lo <= t* <= t_hi of the row system (see the module docstring)."""
    from scipy import sparse
    from scipy.optimize import linprog

    G, h, Aeq, beq = (np.asarray(a, dtype=np.float64) for a in (G, h, Aeq, beq))
    nv = len(lb)
    rows_i, rows_v, rhs = [], [], []
    gi, gv = _sparse_rows(G)
    for ix, v, b in zip(gi, gv, h):
        if len(ix):
            rows_i.append(ix), rows_v.append(v), rhs.append(b)
    for j in range(nv):  # the variable bounds as rows
        if np.isfinite(ub[j]):
            rows_i.append(np.array([j])), rows_v.append(np.array([1.0])), rhs.append(ub[j])
        if np.isfinite(lb[j]):
            rows_i.append(np.array([j])), rows_v.append(np.array([-1.0])), rhs.append(-lb[j])
    m = len(rhs)
    rhs = np.array(rhs)
    nrm = np.array([math.sqrt(float(np.dot(v, v))) for v in rows_v])
    # ---- the LP: variables (x, t), min t, G~ x - t <= h~, Aeq x = beq ------------------------------------------------------------------
    ri = np.concatenate(rows_i + [np.full(m, nv)])
    rr = np.concatenate([np.full(len(ix), i) for i, ix in enumerate(rows_i)] + [np.arange(m)])
    rv = np.concatenate([v / n for v, n in zip(rows_v, nrm)] + [np.full(m, -1.0)])
    A_ub = sparse.csr_matrix((rv, (rr, ri)), shape=(m, nv + 1))
    A_eq = sparse.csr_matrix(np.hstack([Aeq, np.zeros((Aeq.shape[0], 1))])) if len(beq) else None
    for method in ("highs", "highs-ds", "highs-ipm"):  # (the bounds below hold whichever method found the point and the dual)
        res = linprog(np.r_[np.zeros(nv), 1.0], A_ub=A_ub, b_ub=rhs / nrm, A_eq=A_eq, b_eq=beq if len(beq) else None,
                      bounds=[(None, None)] * (nv + 1), method=method)
        if res.status == 0:
            break
    if res.status != 0:
        raise RuntimeError("feasibility LP: %s" % res.message)
    mp = mpmath.mp
    old = mp.dps
    mp.dps = _DPS
    try:
        F = mpmath.mpf
        ei, ev = _sparse_rows(Aeq)
        ev = [[F(float(a)) for a in v] for v in ev]
        rows_m = [[F(float(a)) for a in v] for v in rows_v]
        nrm_m = [mpmath.sqrt(mpmath.fsum(a * a for a in v)) for v in rows_m]
        rhs_m = [F(float(b)) for b in rhs]
        beq_m = [F(float(b)) for b in beq]
        # ---- t_hi: the LP's point on Aeq x = beq to ~1e-45, its largest row residual --------------------------------------------------
        xp = [F(float(a)) for a in res.x[:nv]]
        AAt = Aeq @ Aeq.T if len(beq) else None
        for _ in range(6):
            if not len(beq):
                break
            rho = [mpmath.fsum(a * xp[j] for a, j in zip(v, ix)) - b for v, ix, b in zip(ev, ei, beq_m)]
            rmax = max(abs(r) for r in rho)
            if rmax <= F(10) ** -40:
                break
            w = np.linalg.lstsq(AAt, np.array([float(r) for r in rho]), rcond=None)[0]
            for k, (v, ix) in enumerate(zip(ev, ei)):
                wk = F(float(w[k]))
                for a, j in zip(v, ix):
                    xp[j] -= a * wk
        else:
            rmax = F(0)
        if len(beq) and rmax > F(10) ** -40:
            t_hi = math.inf  # (not projected: no certificate)
        else:
            t_hi = float(max((mpmath.fsum(a * xp[j] for a, j in zip(v, ix)) - b) / n for v, ix, b, n in zip(rows_m, rows_i, rhs_m, nrm_m)))
        # ---- t_lo: weak duality on the LP's multipliers, their residual bounded by the implied box ----------------------------------
        y = np.maximum(-np.asarray(res.ineqlin.marginals, dtype=np.float64), 0.0)
        z = -np.asarray(res.eqlin.marginals, dtype=np.float64) if len(beq) else np.zeros(0)
        ysum = mpmath.fsum(F(float(a)) for a in y)
        if ysum <= 0:
            return Verdict(-math.inf, t_hi, float(res.x[nv]))
        ym = [F(float(a)) / ysum for a in y]
        zm = [F(float(a)) for a in z]
        rho = [F(0)] * nv
        for yi, v, ix, n in zip(ym, rows_m, rows_i, nrm_m):
            if yi:
                for a, j in zip(v, ix):
                    rho[j] += yi * a / n
        for zk, v, ix in zip(zm, ev, ei):
            if zk:
                for a, j in zip(v, ix):
                    rho[j] += zk * a
        dual = -mpmath.fsum(yi * b / n for yi, b, n in zip(ym, rhs_m, nrm_m) if yi) - mpmath.fsum(zk * b for zk, b in zip(zm, beq_m))
        # the box: single-variable rows; pinned: variables the equality rows determine (their value is the same at every such point)
        lo_b, hi_b = np.full(nv, -np.inf), np.full(nv, np.inf)
        for v, ix, b in zip(rows_v, rows_i, rhs):
            if len(ix) == 1:
                if v[0] > 0:
                    hi_b[ix[0]] = min(hi_b[ix[0]], b / v[0])
                else:
                    lo_b[ix[0]] = max(lo_b[ix[0]], b / v[0])
        pinned = np.zeros(nv, bool)
        if len(beq):
            _, s, Vt = np.linalg.svd(Aeq)
            rank = int((s > 1e-10 * s[0]).sum())
            Nsp = Vt[rank:].T
            pinned = np.abs(Nsp).max(axis=1) <= 1e-12 if Nsp.shape[1] else np.ones(nv, bool)
        low = dual
        for j in range(nv):
            if not rho[j]:
                continue
            if pinned[j]:
                low += rho[j] * xp[j]
            else:
                B = max(abs(lo_b[j]), abs(hi_b[j])) + _T_BOX
                if not math.isfinite(B):
                    return Verdict(-math.inf, t_hi, float(res.x[nv]))
                low -= abs(rho[j]) * F(B)
        t_lo = min(_T_BOX, float(low))
    finally:
        mp.dps = old
    return Verdict(t_lo, t_hi, float(res.x[nv]))


def judge_model(model):
    return judge(model["G"], model["h"], model["Aeq"], model["beq"], model["lb"], model["ub"])


# ---- ABI instances <-> the oracle's row-for-row model ---------------------------------------------------------------------------------


def oracle_inputs(O, hdr1, rows1, sfc1):
    """One instance in ABI form (header record, its n_obs * M * 6 rows, its M corridor boxes) -> (agent, lsc, sfc) of oracle/oracle.py.
    The rows go in as they are: normal = (nx, ny, nz), d = b, p = 0 (tests/test_round6_host.py does the same)."""
    ag = np.zeros(1, O.AGENT_DTYPE)
    for f in ("p0", "v0", "a0", "goal", "next_waypoint", "vmax", "amax", "radius", "nominal_velocity", "n_obs"):
        ag[f][0] = hdr1[f]
    lsc = np.zeros(len(rows1), O.LSC_DTYPE)
    lsc["nrm"][:, 0], lsc["nrm"][:, 1], lsc["nrm"][:, 2], lsc["d"] = rows1["nx"], rows1["ny"], rows1["nz"], rows1["b"]
    sfc = np.zeros(len(sfc1), O.BOX_DTYPE)
    sfc["bmin"], sfc["bmax"] = sfc1["bmin"], sfc1["bmax"]
    return ag, lsc, np.ascontiguousarray(sfc)


def judge_instance(O, cls, inst):
    ag, lsc, sfc = oracle_inputs(O, inst.hdr, inst.rows, inst.sfc)
    return judge_model(O.assemble(cls, ag, lsc, sfc))


# ---- the families ---------------------------------------------------------------------------------------------------------------------

EPS_GRID = (1e-8, 3e-7, 8e-7, 1e-6, 2e-6, 1e-5)
DELTA_GRID = (5e-7, 1.05e-6, 1.5e-6, 3e-6, 1e-5, 1e-4)  # (1e-4: beyond every reach at eps <= 1e-6 -- a provably empty pair)
SLAB_WIDTHS = (1e-3, 1e-5, 1e-6, 1e-7, 0.0, -1e-7, -1e-6, -1e-5, -1e-3, -0.4)
EMPTY_GAPS = (1e-12, 1e-9, 1e-6, 1e-3, 0.0)  # bmin - bmax on one axis of one segment (0: a zero-width interval)
OPEN_WIDTHS = (1e-2, 1e-1)                    # narrow open intervals beside them (controls)


class Instance:
    """One QP in ABI form plus what made it.  hdr: HEADER_DTYPE record; rows: ROW_DTYPE[n_obs * M * 6]; sfc: BOX_DTYPE[M]."""
    __slots__ = ("family", "params", "hdr", "rows", "sfc", "verdict")

    def __init__(self, family, params, hdr, rows, sfc):
        self.family, self.params, self.hdr, self.rows, self.sfc, self.verdict = family, params, hdr, rows, sfc, None

    @property
    def label(self):
        return self.verdict.label

    @property
    def kind3_window(self):
        p = self.params
        return self.family == "A" and p["eps"] <= 1e-6 and p["delta"] > 1e-6


def _base(hdr, rows, sfc, q, n_obs, M):
    P = M * 6
    return hdr[q].copy(), rows.reshape(-1, n_obs * P)[q].copy(), sfc.reshape(-1, M)[q].copy()


def _perp(rng, n, dim):
    """A random unit direction orthogonal to n (in the xy plane for dim 2), scaled to |n|."""
    for _ in range(100):
        u = rng.standard_normal(3)
        if dim == 2:
            u[2] = 0.0
        u -= n * (u @ n) / (n @ n)
        if np.linalg.norm(u) > 1e-3:
            return u / np.linalg.norm(u) * np.linalg.norm(n)
    raise RuntimeError("no orthogonal direction")


def _horizontal(rng, n, dim):
    """A unit direction orthogonal to n in the horizontal plane (the world's long axes), scaled to |n|."""
    if dim == 2:
        return _perp(rng, n, dim)
    u = np.cross(n, [0.0, 0.0, 1.0])
    if np.linalg.norm(u) < 1e-3 * np.linalg.norm(n):
        return _perp(rng, n, dim)
    return u / np.linalg.norm(u) * np.linalg.norm(n)


def _toward_centre(u, p0, world_min, world_max, sign=1.0):
    """u or -u: the one along which sign * u points from p0 towards the world's centre (where there is room to travel)."""
    c = 0.5 * (np.asarray(world_min, dtype=np.float64) + np.asarray(world_max, dtype=np.float64)) - p0
    return u if sign * (u @ c) >= 0 else -u


def _open_up(h1, R, s1, world_min, world_max, fast, keep=()):
    """The 'fast' form of an instance: vmax, amax raised, every corridor box the world box, every LSC row cleared (a zero normal: the row is
    dropped) except those of `keep` ((neighbour, control point) pairs, or neighbour indices) -- room for a control point to travel."""
    h1["vmax"], h1["amax"] = fast
    for k in range(3):
        s1["bmin"][:, k], s1["bmax"][:, k] = world_min[k], world_max[k]
    mask = np.ones(R.shape, bool)
    for kp in keep:
        mask[kp] = False
    for f in ("nx", "ny", "nz", "b"):
        R[f][mask] = 0.0


def family_a(hdr, rows, sfc, n_obs, M, dim, world_min, world_max, seed, fast=(5.0, 20.0), reps=1, variants=("base", "fast", "face")):
    """Near-antiparallel pairs.  For each (eps, delta) of the grid and each variant: one control point j of a late segment (the last two) of
    a swarm instance gets, in place of neighbour 1's row there, the row of neighbour 0 reversed and tilted:
        n0.c >= b0     and     (n0 + eps u).(c - p0) <= b0 - n0.p0 - delta       (u orthogonal to n0, |u| = |n0|)
    -- antiparallel up to eps, overlapping by delta at every point of the plane u.(c - p0) = 0; a common point lies delta / eps along -u.
    Variants: 'base' (the swarm's own limits, corridor and neighbours); 'fast' (_open_up: raised limits, the world as corridor, neighbour 0
    and the pair alone); 'face' (as 'fast', but the partner is the upper corridor face on one axis k of j's segment, n = e_k + eps u, and no
    LSC row but the partner)."""
    rng = np.random.default_rng(seed)
    P = M * 6
    N = len(hdr)
    out = []
    for variant in variants:
        for eps in EPS_GRID:
            for delta in DELTA_GRID:
                for _ in range(reps):
                    q = int(rng.integers(N))
                    h1, r1, s1 = _base(hdr, rows, sfc, q, n_obs, M)
                    R = r1.reshape(n_obs, P)
                    cand = [j for j in range(P - 12, P) if (R["nx"][0, j], R["ny"][0, j], R["nz"][0, j]) != (0.0, 0.0, 0.0)]
                    j = int(rng.choice(cand)) if cand and variant == "base" else P - 1  # (the open forms: the last control point, the farthest reach)
                    seg = j // 6
                    p0 = np.array(h1["p0"], dtype=np.float64)
                    if variant == "face":
                        _open_up(h1, R, s1, world_min, world_max, fast, keep=[(1, j)])
                        k = int(rng.integers(dim))
                        box = h1["p0"][k] + np.array([-0.3, 0.3])  # j's segment keeps a corridor on axis k about p0
                        s1["bmin"][seg][k], s1["bmax"][seg][k] = box
                        e = np.zeros(3)
                        e[k] = 1.0
                        u = _toward_centre(_perp(rng, e, dim), p0, world_min, world_max)
                        n1 = e + eps * u
                        # n1.(c - p0) >= bmax_k - p0_k + delta: beyond the face by delta, unless c moves delta / eps along u
                        b1 = float(s1["bmax"][seg][k]) - p0[k] + delta + n1 @ p0
                        R["nx"][1, j], R["ny"][1, j], R["nz"][1, j], R["b"][1, j] = n1[0], n1[1], n1[2], b1
                    else:
                        if variant == "fast":
                            _open_up(h1, R, s1, world_min, world_max, fast, keep=[0])
                        n0 = np.array([R["nx"][0, j], R["ny"][0, j], R["nz"][0, j]])
                        b0 = float(R["b"][0, j])
                        u = _perp(rng, n0, dim)
                        if variant == "fast":
                            u = _toward_centre(_horizontal(rng, n0, dim), p0, world_min, world_max, sign=-1.0)
                        n1 = n0 + eps * u
                        # -(n1).c >= -(b0 - n0.p0 - delta + n1.p0)
                        R["nx"][1, j], R["ny"][1, j], R["nz"][1, j] = -n1[0], -n1[1], -n1[2]
                        R["b"][1, j] = -(b0 - n0 @ p0 - delta + n1 @ p0)
                    out.append(Instance("A", dict(variant=variant, eps=eps, delta=delta, q=q, j=j), h1, R.reshape(-1), s1))
    return out


def family_b(hdr, rows, sfc, n_obs, M, dim, world_min, world_max, seed, fast=(5.0, 20.0), reps=2):
    """Graded slabs: neighbour 1's rows become neighbour 0's mirrored to a slab of width w, n.c >= b and n.c <= b + w (bench.make_infeasible
    is w = -0.4) -- on every control point ('all'), on the last segment's only ('late'), or on those in the open form of _open_up
    ('late_fast': a slab the trajectory can reach, so that the marginally open ones are feasible)."""
    rng = np.random.default_rng(seed)
    P = M * 6
    out = []
    for scope in ("all", "late", "late_fast"):
        for w in SLAB_WIDTHS:
            for _ in range(reps):
                q = int(rng.integers(len(hdr)))
                h1, r1, s1 = _base(hdr, rows, sfc, q, n_obs, M)
                R = r1.reshape(n_obs, P)
                js = np.arange(P) if scope == "all" else np.arange(P - 6, P)
                if scope == "late_fast":
                    _open_up(h1, R, s1, world_min, world_max, fast, keep=[0])
                for f in ("nx", "ny", "nz"):
                    R[f][1, js] = -R[f][0, js]
                R["b"][1, js] = -R["b"][0, js] - w
                out.append(Instance("B", dict(scope=scope, w=w, q=q), h1, R.reshape(-1), s1))
    return out


def family_c(hdr, rows, sfc, n_obs, M, dim, seed, reps=2):
    """Empty (bmin - bmax = g > 0), zero-width (g = 0) and narrow open (width OPEN_WIDTHS) corridor intervals on one axis of one segment, about
    the centre of that segment's box."""
    rng = np.random.default_rng(seed)
    out = []
    for g in EMPTY_GAPS + tuple(-w for w in OPEN_WIDTHS):
        for _ in range(reps):
            q = int(rng.integers(len(hdr)))
            h1, r1, s1 = _base(hdr, rows, sfc, q, n_obs, M)
            m, k = int(rng.integers(1, M)), int(rng.integers(dim))
            c = 0.5 * (float(s1["bmin"][m][k]) + float(s1["bmax"][m][k]))
            if g == 0.0:
                s1["bmin"][m][k] = s1["bmax"][m][k] = c
            else:
                s1["bmin"][m][k], s1["bmax"][m][k] = c + 0.5 * g, c - 0.5 * g
            out.append(Instance("C", dict(gap=g, seg=m, axis=k, q=q), h1, r1, s1))
    return out


# (M, dim, n_obs).  "generic": the shape kept its name from round 3, when M = 9 in 3-D had no compiled instance; it has one since (14
# neighbours), so only the forced path of tests/test_infeasible_verdicts.py runs it on the run-time-shaped kernel.  "m12": no compiled
# instance at all -- every path that reaches an interior-point kernel ends in the run-time-shaped one.
SHAPES = {"c1": (5, 3, 8), "c0": (10, 2, 8), "generic": (9, 3, 8), "m12": (12, 3, 8)}


class Group:
    """Instances of one solver class: the swarm's own ('swarm'), or the open world ('open': the world box 10 m wider on every side and no
    communication-range rows, comm_range = 0 -- where a control point can travel far enough for the kind-3 window to hold feasible pairs)."""

    def __init__(self, name, M, dim, n_obs, world_min, world_max, comm_range, insts):
        self.name, self.M, self.dim, self.n_obs = name, M, dim, n_obs
        self.world_min, self.world_max, self.comm_range, self.insts = tuple(world_min), tuple(world_max), comm_range, insts

    def oracle_class(self, O):
        return O.make_class(M=self.M, dim=self.dim, comm_range=self.comm_range, world_min=self.world_min, world_max=self.world_max)

    def desc(self, api, **kw):
        return api.make_desc(M=self.M, dim=self.dim, comm_range=self.comm_range, world_min=self.world_min, world_max=self.world_max, **kw)


def build_groups(api, O, shape, seed=5, judge_all=True):
    """The families on one shape (SHAPES), generated from a synth swarm's first replan and labelled by the referee."""
    from lsc_dr_planner_amd import synth

    M, dim, n_obs = SHAPES[shape]
    sw = synth.Swarm(16, M=M, dim=dim, n_obs=n_obs, seed=seed)
    hdr, rows, _, sfc = api.batch_from_swarm(sw.build(), sw.n_obs, M)
    wmin, wmax = np.asarray(sw.world_min, dtype=np.float64), np.asarray(sw.world_max, dtype=np.float64)
    swarm = family_a(hdr, rows, sfc, n_obs, M, dim, wmin, wmax, seed + 1, variants=("base",))
    swarm += family_b(hdr, rows, sfc, n_obs, M, dim, wmin, wmax, seed + 2, reps=1)
    swarm += family_c(hdr, rows, sfc, n_obs, M, dim, seed + 3, reps=1)
    owmin, owmax = wmin - 10.0, wmax + 10.0
    opened = family_a(hdr, rows, sfc, n_obs, M, dim, owmin, owmax, seed + 4, variants=("fast",), reps=2)
    opened += family_a(hdr, rows, sfc, n_obs, M, dim, owmin, owmax, seed + 5, variants=("face",), reps=1)
    groups = [Group("swarm", M, dim, n_obs, wmin, wmax, 3.0, swarm), Group("open", M, dim, n_obs, owmin, owmax, 0.0, opened)]
    if judge_all:
        for g in groups:
            cls = g.oracle_class(O)
            for i in g.insts:
                i.verdict = judge_instance(O, cls, i)
    return groups


def to_batch(api, insts, n_obs, M):
    """A list of instances -> (hdr, rows, row_offsets, sfc) of one call."""
    hdr = np.concatenate([np.atleast_1d(i.hdr) for i in insts]).astype(api.HEADER_DTYPE)
    rows = np.concatenate([i.rows for i in insts]).astype(api.ROW_DTYPE)
    off = np.arange(len(insts) + 1, dtype=np.uint64) * np.uint64(n_obs * M * 6)
    sfc = np.concatenate([i.sfc for i in insts]).astype(api.BOX_DTYPE)
    return hdr, rows, off, sfc


def label_counts(insts, key=lambda i: i.family):
    c = Counter()
    for i in insts:
        c[(key(i), i.label)] += 1
    return c
