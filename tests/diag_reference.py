"""A numpy restatement of lscqp_diagnose (include/lscqp.h, "failure diagnostics"), row by row.

Written from the header's description of the record and from the reference's TrajOptimizer::populatebyrow
(src/traj_optimizer.cpp:238-511), not from the kernel: every row of the model is kept as the reference adds it -- a list of
(axis, segment, point, coefficient) terms, a sense and a right-hand side -- and evaluated in plain fp64, one product and one
addition at a time.  Nothing is fused, reordered or vectorised, so the figures are what `G x - h`, `|Aeq x - beq|` and
`max(lb - x, x - ub)` of the oracle's assembly give (tests/test_diag.py holds the two together).

A NAME (family, obstacle, segment, point, axis) stands for one reference row, or for the `+` / `-` pair of rows the reference adds
for a two-sided limit; its value is the larger of the pair, in the units the header states.  Within a family the names come in
populatebyrow order.  Fields that do not apply are -1:

    BOUND          (-1, m, i, k)   lb <= x <= ub of control point i of segment m on axis k         order k, m, i
    SFC            (-1, m, i, k)   the two faces of segment m's corridor on axis k                 order m, k, i
    LSC            (oi, m, i, -1)  n.c >= b of obstacle slot oi                                    order oi, m, i
    VEL            (-1, m, i, k)   |5/dt (c[i+1] - c[i])| <= vmax[k]                               order k, m, i
    ACC            (-1, m, i, k)   |20/dt^2 (c[i+2] - 2 c[i+1] + c[i])| <= amax[k]                 order k, m, i
    COMM_PAIR      (mi, m, 5, k)   |c[m][5] - c[mi][0]| <= R/2 - radius, mi <= m                   order k, mi, m
    COMM_WAYPOINT  (-1, m, 5, k)   |c[m][5] - waypoint| <= R/2 - 1e-5                              order k, m
    EQUALITY       (-1, m, j, k)   m = 0: j = 0, 1, 2 initial position / velocity / acceleration; m >= 1: j = 0, 1, 2 the C0 / C1 / C2
                                   join of segment m - 1 to m; (M - 1, 4) and (M - 1, 3) the end stop c5 = c4, c5 = c3
                                   order: per k (0,0) (1,0) (0,1) (0,2) (1,1) (1,2); per k, m >= 2, j; per k (M-1,4) (M-1,3)

The record (DIAG_DTYPE) follows the two rules the header states: among rows of equal violation the named row is the least in
(family, obstacle, segment, point, axis); a row whose value is NaN or +inf counts as violated with value +inf.
"""
import math
from collections import namedtuple

import numpy as np

BOUND, SFC, LSC, VEL, ACC, COMM_PAIR, COMM_WAYPOINT, EQUALITY, FAMILIES = range(9)
PLANNER_DLSC, PLANNER_LSC, PLANNER_BVC, PLANNER_RSFC = 0, 1, 2, 3
DIAG_DTYPE = np.dtype([("worst", "f8", 8), ("violated", "i4", 8), ("violation", "f8"), ("family", "i4"), ("obstacle", "i4"),
                       ("segment", "i4"), ("point", "i4"), ("axis", "i4"), ("reserved", "i4")])
EPS_SHORT_NORMAL = 1e-5  # :409-411
U = 2.0 ** -52

Class = namedtuple("Class", "M dim dt planner use_sfc comm_range world_min world_max")
Row = namedtuple("Row", "family obstacle segment point axis value scale")
# one reference row: terms (k, m, i, coefficient); sense "<=", ">=" or "="
ModelRow = namedtuple("ModelRow", "terms sense rhs")


def make_class(M=5, dim=3, dt=0.2, planner=PLANNER_LSC, use_sfc=True, comm_range=3.0, world_min=(-5, -5, 0), world_max=(5, 5, 2.5)):
    return Class(int(M), int(dim), float(dt), int(planner), bool(use_sfc), float(comm_range), tuple(float(v) for v in world_min),
                 tuple(float(v) for v in world_max))


def bound(scale):
    """The tolerance of every comparison with this restatement: 8 * 2^-52 * scale (tests/test_diag.py, module docstring)."""
    return 8.0 * U * scale


def evaluate(row, X):
    """(violation, scale) of one reference row on the control points X[k, m, i]: positive = violated; `=` rows give |residual|."""
    lhs, scale = 0.0, abs(row.rhs)
    for k, m, i, a in row.terms:
        t = a * float(X[k, m, i])
        lhs += t
        scale += abs(t)
    if row.sense == "<=":
        return lhs - row.rhs, scale
    if row.sense == ">=":
        return row.rhs - lhs, scale
    return abs(lhs - row.rhs), scale


def model(cls, hdr, rows, boxes):
    """The reference's model of ONE instance, in populatebyrow order within each family:
    ([(family, obstacle, segment, point, axis, (ModelRow, ...))], number of LSC rows skipped for a short normal).
    hdr: one header record; rows: (n_obs, M, 6) packed rows (nx, ny, nz, b) in the values the handle reads, or None;
    boxes: (M,) corridor boxes, or None when the class carries no SFC rows."""
    M, dim, dt = cls.M, cls.dim, cls.dt
    sv, sa = 5.0 / dt, 20.0 / (dt * dt)
    fixed = lambda m, i: m == 0 and i < 3  # the initial state: free variables, no row (:252-253, :404-406)
    out, skipped = [], 0
    for k in range(dim):  # :238-270
        for m in range(M):
            for i in range(6):
                if fixed(m, i):
                    continue
                lo, hi = cls.world_min[k], cls.world_max[k]
                if cls.planner == PLANNER_RSFC and k == 2 and m == 0:  # :255-258
                    lo, hi = -100.0, 100.0
                out.append((BOUND, -1, m, i, k, (ModelRow(((k, m, i, 1.0),), ">=", lo), ModelRow(((k, m, i, 1.0),), "<=", hi))))
    if cls.use_sfc:  # :372-397, faces per axis: +e_k at box_min, then -e_k at box_max
        for m in range(M):
            for k in range(dim):
                for i in range(6):
                    if fixed(m, i):
                        continue
                    out.append((SFC, -1, m, i, k, (ModelRow(((k, m, i, 1.0),), ">=", float(boxes[m]["bmin"][k])),
                                                   ModelRow(((k, m, i, -1.0),), ">=", -float(boxes[m]["bmax"][k])))))
    for oi in range(int(hdr["n_obs"])):  # :399-437
        for m in range(M):
            for i in range(6):
                if fixed(m, i):
                    continue
                r = rows[oi, m, i]
                nrm = (float(r["nx"]), float(r["ny"]), float(r["nz"]))
                if math.sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]) < EPS_SHORT_NORMAL:
                    skipped += 1
                    continue
                out.append((LSC, oi, m, i, -1, (ModelRow(tuple((k, m, i, nrm[k]) for k in range(dim)), ">=", float(r["b"])),)))
    vel, acc = [], []
    for k in range(dim):  # :439-474
        vmax, amax = float(hdr["vmax"][k]), float(hdr["amax"][k])
        for m in range(M):
            for i in range(5):
                if m == 0 and i < 2:
                    continue
                vel.append((VEL, -1, m, i, k, (ModelRow(((k, m, i + 1, sv), (k, m, i, -sv)), "<=", vmax),
                                               ModelRow(((k, m, i + 1, -sv), (k, m, i, sv)), "<=", vmax))))
            for i in range(4):
                if m == 0 and i < 1:
                    continue
                acc.append((ACC, -1, m, i, k, (ModelRow(((k, m, i + 2, sa), (k, m, i + 1, -2.0 * sa), (k, m, i, sa)), "<=", amax),
                                               ModelRow(((k, m, i + 2, -sa), (k, m, i + 1, 2.0 * sa), (k, m, i, -sa)), "<=", amax))))
    out += vel + acc
    if cls.comm_range > 0:  # :476-500
        rho, rho_w = 0.5 * cls.comm_range - float(hdr["radius"]), 0.5 * cls.comm_range - 1e-5
        for k in range(dim):
            for mi in range(M):
                for m in range(mi, M):
                    out.append((COMM_PAIR, mi, m, 5, k, (ModelRow(((k, m, 5, 1.0), (k, mi, 0, -1.0)), "<=", rho),
                                                         ModelRow(((k, m, 5, -1.0), (k, mi, 0, 1.0)), "<=", rho))))
        for k in range(dim):
            w = float(hdr["next_waypoint"][k])
            for m in range(M):
                out.append((COMM_WAYPOINT, -1, m, 5, k, (ModelRow(((k, m, 5, 1.0),), "<=", rho_w + w), ModelRow(((k, m, 5, -1.0),), "<=", rho_w - w))))
    eq = lambda m, j, k, terms, rhs=0.0: out.append((EQUALITY, -1, m, j, k, (ModelRow(tuple(terms), "=", rhs),)))
    assert M >= 2
    for k in range(dim):  # :318-353: the initial state and the first join, which the reference leaves unscaled
        eq(0, 0, k, [(k, 0, 0, 1.0)], float(hdr["p0"][k]))
        eq(1, 0, k, [(k, 0, 5, 1.0), (k, 1, 0, -1.0)])
        eq(0, 1, k, [(k, 0, 1, sv), (k, 0, 0, -sv)], float(hdr["v0"][k]))
        eq(0, 2, k, [(k, 0, 2, sa), (k, 0, 1, -2.0 * sa), (k, 0, 0, sa)], float(hdr["a0"][k]))
        eq(1, 1, k, [(k, 1, 1, 1.0), (k, 1, 0, -1.0), (k, 0, 5, -1.0), (k, 0, 4, 1.0)])
        eq(1, 2, k, [(k, 1, 2, 1.0), (k, 1, 1, -2.0), (k, 1, 0, 1.0), (k, 0, 5, -1.0), (k, 0, 4, 2.0), (k, 0, 3, -1.0)])
    for k in range(dim):  # :356-368 with buildAeqBase (:180-214): the later joins, derivative j scaled by dt^-j n!/(n-j)!
        for m in range(2, M):
            eq(m, 0, k, [(k, m - 1, 5, 1.0), (k, m, 0, -1.0)])
            eq(m, 1, k, [(k, m - 1, 5, sv), (k, m - 1, 4, -sv), (k, m, 1, -sv), (k, m, 0, sv)])
            eq(m, 2, k, [(k, m - 1, 5, sa), (k, m - 1, 4, -2.0 * sa), (k, m - 1, 3, sa), (k, m, 2, -sa), (k, m, 1, 2.0 * sa), (k, m, 0, -sa)])
    if cls.planner == PLANNER_LSC:  # :502-511
        for k in range(dim):
            for j in (1, 2):
                eq(M - 1, 5 - j, k, [(k, M - 1, 5, 1.0), (k, M - 1, 5 - j, -1.0)])
    return out, skipped


def rows_of(cls, hdr, rows, boxes, x):
    """Every name of ONE instance as Row(family, obstacle, segment, point, axis, value, scale), in populatebyrow order within each
    family, and the number of skipped short-normal rows.  x: (dim * 6M,) in the reference variable order x[k * 6M + 6m + i]."""
    X = np.asarray(x, dtype=np.float64).reshape(cls.dim, cls.M, 6)
    names, skipped = model(cls, hdr, rows, boxes)
    out = []
    for fam, obs, seg, pt, ax, mrows in names:
        ev = [evaluate(r, X) for r in mrows]
        vals = [v for v, _ in ev]
        value = float("nan") if any(v != v for v in vals) else max(vals)  # (a NaN in either row of a pair makes the name NaN)
        out.append(Row(fam, obs, seg, pt, ax, value, max(s for _, s in ev)))
    return out, skipped


def effective(v):
    """The value a row counts with: NaN and +inf are +inf (include/lscqp.h, the non-finite rule)."""
    return math.inf if v != v else v


def key(r):
    return (r.family, r.obstacle, r.segment, r.point, r.axis)


def argmax_set(rows):
    """The rows that share the largest effective value, least key first."""
    if not rows:
        return []
    top = max(effective(r.value) for r in rows)
    return sorted((r for r in rows if effective(r.value) == top), key=key)


def runner_up(rows):
    """The largest effective value among the rows outside the argmax set (-inf if there is none)."""
    top = set(key(r) for r in argmax_set(rows))
    rest = [effective(r.value) for r in rows if key(r) not in top]
    return max(rest) if rest else -math.inf


def family_scale(rows, fam):
    """The largest scale in a family: what bounds |worst[fam]| of the kernel against this restatement."""
    s = [r.scale for r in rows if r.family == fam]
    return max(s) if s else 0.0


def record(rows, tol):
    """The DIAG_DTYPE record of one instance from its list of rows."""
    d = np.zeros((), DIAG_DTYPE)
    for f in range(FAMILIES):
        ev = [effective(r.value) for r in rows if r.family == f]
        d["worst"][f] = max(ev) if ev else 0.0
        d["violated"][f] = sum(1 for v in ev if v > tol)
    best = argmax_set(rows)
    if best:
        b = best[0]
        d["violation"] = effective(b.value)
        d["family"], d["obstacle"], d["segment"], d["point"], d["axis"] = key(b)
    else:
        d["family"] = d["obstacle"] = d["segment"] = d["point"] = d["axis"] = -1
    return d


def diagnose(cls, hdr, rows, row_offsets, sfc, x, tol):
    """lscqp_diagnose restated: (DIAG_DTYPE[n], [rows of instance q], [skipped of instance q]).  rows: the flat packed rows the handle
    reads (f32 rows already widened), instance q's at row_offsets[q] .. + n_obs * 6M; sfc: (n, M) boxes or None; x: (n, nv)."""
    n, P = len(hdr), 6 * cls.M
    out, lists, skipped = np.zeros(n, DIAG_DTYPE), [], []
    for q in range(n):
        n_obs = int(hdr[q]["n_obs"])
        rq = None
        if n_obs > 0:
            r0 = int(row_offsets[q])
            rq = np.asarray(rows).reshape(-1)[r0:r0 + n_obs * P].reshape(n_obs, cls.M, 6)
        bq = None if sfc is None or not cls.use_sfc else np.asarray(sfc).reshape(n, cls.M)[q]
        L, s = rows_of(cls, hdr[q], rq, bq, np.asarray(x).reshape(n, -1)[q])
        out[q] = record(L, tol)
        lists.append(L)
        skipped.append(s)
    return out, lists, skipped
