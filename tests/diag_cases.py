"""Instances for tests/test_diag.py: the five classes lscqp_diagnose is held to, random batches, and trajectories on which ONE chosen
row of the reference's model is the unique worst.  numpy only; the rows come from tests/diag_reference.py."""
import numpy as np

from tests import diag_reference as R

# (M, dim, planner, use_sfc, communication range, n_obs)
CLASSES = [(5, 3, "LSC", True, 3.0, 4), (10, 2, "LSC", True, 3.0, 2), (4, 3, "DLSC", True, 0.0, 3), (10, 3, "RSFC", False, 3.0, 7),
           (5, 2, "DLSC", True, 3.0, 0)]
CLASS_IDS = ["M%d_dim%d_%s_sfc%d_range%g_obs%d" % (M, dim, p, s, r, o) for M, dim, p, s, r, o in CLASSES]
_API_MODE = {"LSC": R.PLANNER_LSC, "DLSC": R.PLANNER_DLSC, "RSFC": R.PLANNER_RSFC}  # (lscqp_class_desc.planner_mode)
_ORACLE_MODE = {"LSC": 1, "DLSC": 0, "RSFC": 2}  # oracle.make_class(planner_lsc=...)
# random trajectories live in +-3: a world box they leave on every axis.  Pushed rows start from a hover at HOVER, a point with exactly
# representable margins to every face of WORLD_WIDE.
WORLD_TIGHT = ((-2.0, -2.5, 0.0), (2.5, 2.0, 2.5))
WORLD_WIDE = ((-6.0, -5.0, -4.0), (5.0, 6.0, 4.5))
HOVER = np.array([-0.5, 0.5, 0.25])
DT = 0.2


def api():
    """lsc_dr_planner_amd.api, imported on use: the struct layouts, make_desc and Solver.  (A test takes the library itself through the `api`
    fixture, which builds a missing one first; nothing here loads it at import.)"""
    from lsc_dr_planner_amd import api as A

    return A


def ref_class(spec, world=WORLD_TIGHT):
    M, dim, planner, use_sfc, rng, _ = spec
    return R.make_class(M=M, dim=dim, dt=DT, planner=_API_MODE[planner], use_sfc=use_sfc, comm_range=rng, world_min=world[0], world_max=world[1])


def solver(spec, world=WORLD_TIGHT, row_format=0):
    """A handle of the class; row_format: LSCQP_ROWS_F64 (0) or LSCQP_ROWS_F32."""
    M, dim, planner, use_sfc, rng, _ = spec
    A = api()
    return A.Solver(A.make_desc(M=M, dim=dim, dt=DT, comm_range=rng, planner_mode=_API_MODE[planner], use_sfc=use_sfc, world_min=world[0],
                                world_max=world[1], row_format=row_format))


def oracle_class(oracle, spec, world=WORLD_TIGHT):
    M, dim, planner, use_sfc, rng, _ = spec
    return oracle.make_class(M=M, dim=dim, dt=DT, comm_range=rng, planner_lsc=_ORACLE_MODE[planner], use_sfc=use_sfc, world_min=world[0],
                             world_max=world[1])


def offsets(counts, M, gaps=None):
    """row_offsets of instances with `counts` obstacles each; gaps[q] unused rows follow instance q's."""
    off = np.zeros(len(counts) + 1, np.uint64)
    for q, c in enumerate(counts):
        off[q + 1] = off[q] + np.uint64(c * 6 * M + (0 if gaps is None else gaps[q]))
    return off


def random_batch(spec, n, seed, short_normal=True):
    """n instances with every header field, row, box and control point drawn at random; x uniform in +-3.  With short_normal, instance q
    carries one LSC row with |n| = 3e-6 and b = 1e6: the worst row by far if it were a row.  -> hdr, rows (n, n_obs, M, 6), off, sfc, x."""
    A = api()
    M, dim, _, _, _, n_obs = spec
    g = np.random.default_rng(seed)
    hdr = np.zeros(n, A.HEADER_DTYPE)
    for f in ("p0", "v0", "a0", "goal", "next_waypoint"):
        hdr[f] = g.uniform(-1, 1, (n, 3))
    hdr["vmax"], hdr["amax"] = g.uniform(0.5, 1.5, (n, 3)), g.uniform(1, 3, (n, 3))
    hdr["radius"], hdr["nominal_velocity"], hdr["n_obs"] = g.uniform(0.1, 0.3, n), 1.0, n_obs
    rows = np.zeros((n, n_obs, M, 6), A.ROW_DTYPE)
    for f in ("nx", "ny", "nz", "b"):
        rows[f] = g.uniform(-1, 1, rows.shape)
    if short_normal and n_obs:
        for q in range(n):
            o, m, i = q % n_obs, 1 + q % (M - 1), (2 * q + 1) % 6
            u = g.normal(size=3)
            u *= 3e-6 / np.linalg.norm(u)
            rows[q, o, m, i] = (u[0], u[1], u[2], 1e6)
    sfc = np.zeros((n, M), A.BOX_DTYPE)
    sfc["bmin"], sfc["bmax"] = g.uniform(-2, -0.5, (n, M, 3)), g.uniform(0.5, 2, (n, M, 3))
    x = g.uniform(-3, 3, (n, dim * 6 * M))
    return hdr, rows, offsets([n_obs] * n, M), sfc, x


def oracle_inputs(oracle, hdr, rows, sfc):
    """One instance for oracle.assemble: the agent, the LSC records (p = 0, so that d IS the packed row's b) and the boxes."""
    ag = np.zeros(1, oracle.AGENT_DTYPE)
    for f in ("p0", "v0", "a0", "goal", "next_waypoint", "vmax", "amax", "radius", "nominal_velocity", "n_obs"):
        ag[f] = hdr[f]
    lsc = np.zeros(rows.size, oracle.LSC_DTYPE)
    flat = rows.reshape(-1)
    lsc["nrm"][:, 0], lsc["nrm"][:, 1], lsc["nrm"][:, 2], lsc["d"] = flat["nx"], flat["ny"], flat["nz"], flat["b"]
    box = np.zeros(len(sfc), oracle.BOX_DTYPE)
    box["bmin"], box["bmax"] = sfc["bmin"], sfc["bmax"]
    return ag, lsc, box


# ---- one row pushed ------------------------------------------------------------------------------------------------------------------
def wide_world(spec):
    """The world box of the pushed rows.  An RSFC class bounds z of segment 0 by +-100 (:255-258): its world reaches further down, so that -100
    is the bound in reach of segment 0, and stops below +100, so that the later segments can leave it while segment 0 is inside."""
    if spec[2] == "RSFC":
        return ((-6.0, -5.0, -150.0), (5.0, 6.0, 90.0))
    return WORLD_WIDE


def hover_instance(spec, hover, g):
    """A feasible instance with wide margins: every control point at `hover`, at rest, the corridor faces 40 m away, every LSC row satisfied
    by 50, the dynamic limits out of reach.  A case then narrows the one margin it is about.  -> hdr, rows (n_obs, M, 6), sfc (M,), x."""
    A = api()
    M, dim, _, _, _, n_obs = spec
    hdr = np.zeros((), A.HEADER_DTYPE)
    hdr["p0"] = hdr["goal"] = hdr["next_waypoint"] = hover
    hdr["vmax"], hdr["amax"], hdr["radius"], hdr["nominal_velocity"], hdr["n_obs"] = 1e6, 1e6, 0.15, 1.0, n_obs
    rows = np.zeros((n_obs, M, 6), A.ROW_DTYPE)
    nrm = g.uniform(0.5, 1.0, (n_obs, M, 6, 3)) * g.choice([-1.0, 1.0], (n_obs, M, 6, 3))
    rows["nx"], rows["ny"], rows["nz"] = nrm[..., 0], nrm[..., 1], nrm[..., 2]
    rows["b"] = (nrm[..., :dim] * hover[:dim]).sum(-1) - 50.0
    sfc = np.zeros(M, A.BOX_DTYPE)
    sfc["bmin"], sfc["bmax"] = hover - 40.0, hover + 40.0
    x = np.tile(hover[:dim, None], (1, 6 * M)).reshape(-1)
    return hdr, rows, sfc, x


def chosen_rows(spec):
    """The rows to push in one class: (family, obstacle, segment, point, axis, side) with side 0 / 1 the first / second reference row of the
    name (lower / upper face, + / - sign).  Each family in a first, a middle and the last segment, on axis 0 and on the last axis.
    A row can be the UNIQUE worst only where the equalities do not tie it to another: c5 of a segment IS c0 of the next (C0 join), the
    first and last difference of neighbouring segments are equal (C1, C2 joins), and the end stop makes c3 = c4 = c5 of the last segment.
    The single-point rows are therefore taken at interior control points, VEL at i = 1..3 and ACC at i = 1, 2; tests/test_diag.py:
    test_diagnose_tie_rule covers rows that do tie."""
    M, dim, planner, use_sfc, rng, n_obs = spec
    mid, last, kz = M // 2, M - 1, dim - 1
    out = []
    pts = [(0, 3, 0, 0), (0, 4, kz, 1), (mid, 1, kz, 0), (mid, 3, 0, 1), (last, 2, 0, 0), (last, 1, kz, 1)]
    out += [(R.BOUND, -1, m, i, k, s) for m, i, k, s in pts]
    if planner == "RSFC":  # the z bound of segment 0 is -100 there, the world's -150 does not count; the later segments leave through the top
        pts = [(m, i, k, s if k != 2 else int(m > 0)) for m, i, k, s in pts] + [(0, 3, 2, 0)]
        out = [(R.BOUND, -1, m, i, k, s) for m, i, k, s in pts]
    if use_sfc:
        out += [(R.SFC, -1, m, i, k, s) for m, i, k, s in pts]
    if n_obs:
        out += [(R.LSC, o, m, i, -1, 0) for o, (m, i) in zip([0, n_obs - 1, n_obs // 2, n_obs - 1, 0, n_obs - 1],
                                                                [(0, 3), (0, 4), (mid, 2), (mid, 4), (last, 1), (last, 2)])]
    out += [(R.VEL, -1, m, i, k, s) for m, i, k, s in [(0, 2, 0, 0), (0, 3, kz, 1), (mid, 1, kz, 0), (mid, 3, 0, 1), (last, 1, 0, 0), (last, 2, kz, 1)]]
    out += [(R.ACC, -1, m, i, k, s) for m, i, k, s in [(0, 1, 0, 0), (0, 2, kz, 1), (mid, 1, kz, 0), (mid, 2, 0, 1), (last, 2, 0, 0), (last, 1, kz, 1)]]
    if rng > 0:
        out += [(R.COMM_PAIR, mi, m, 5, k, s) for mi, m, k, s in [(0, 0, 0, 0), (0, mid, kz, 1), (mid, last, 0, 1), (last, last, kz, 0), (0, last, kz, 0)]]
        out += [(R.COMM_WAYPOINT, -1, m, 5, k, s) for m, k, s in [(0, 0, 0), (mid, kz, 1), (last, kz, 0), (last, 0, 1)]]
    eqs = [(0, 0, 0), (0, 1, kz), (0, 2, 0), (1, 0, kz), (1, 1, 0), (1, 2, kz), (mid, 0, 0), (mid, 1, kz), (mid, 2, 0), (last, 0, kz), (last, 1, 0),
           (last, 2, kz)]
    if planner == "LSC":
        eqs += [(last, 4, 0), (last, 3, kz), (last, 4, kz)]
    out += [(R.EQUALITY, -1, m, j, k, s) for (m, j, k), s in zip(dict.fromkeys(eqs), [0, 1] * 8)]
    return out


def interior_bound_rows(spec):
    """(BOUND, -1, m, i, k, side) of every interior control coordinate (see chosen_rows): what fills a batch with distinct pushed rows."""
    M, dim = spec[0], spec[1]
    return [(R.BOUND, -1, m, i, k, (m + i + k) % 2) for k in range(dim) for m in range(M) for i in ((3, 4) if m == 0 else (1, 2) if m == M - 1 else (1, 2, 3, 4))]


def _dense(row, cls):
    a = np.zeros(cls.dim * 6 * cls.M)
    for k, m, i, c in row.terms:
        a[k * 6 * cls.M + 6 * m + i] += c
    return a


def pushed_instance(spec, cls, name, g, by=0.3, near=0.25):
    """An instance on whose trajectory `name` = (family, obstacle, segment, point, axis, side) is the one violated row, by `by` in its units.
    The hover instance first gets the margin of that row narrowed to `near` (its face, plane, limit, waypoint or radius; for a variable bound
    the hover itself sits `near` inside the face).  The trajectory then moves by the dx that gives the row its value, keeps every equality
    (or breaks the chosen one alone), and is least-squares smallest on the other rows of the family -- one control point alone cannot do
    that: it takes part in a join, which it would break by at least as much.  -> hdr, rows, sfc, x."""
    fam, obs, seg, pt, ax, side = name
    hover = HOVER.copy()
    if fam == R.BOUND:
        lo, hi = cls.world_min[ax], cls.world_max[ax]
        if cls.planner == R.PLANNER_RSFC and ax == 2 and seg == 0:
            lo, hi = -100.0, 100.0
        hover[ax] = lo + near if side == 0 else hi - near
    hdr, rows, sfc, x = hover_instance(spec, hover, g)
    if fam == R.SFC:
        sfc[seg]["bmin" if side == 0 else "bmax"][ax] = hover[ax] + (-near if side == 0 else near)
    elif fam == R.LSC:
        r = rows[obs, seg, pt]
        r["b"] = sum(float(r[f]) * hover[k] for k, f in enumerate(("nx", "ny", "nz")[:cls.dim])) - near
    elif fam == R.VEL:
        hdr["vmax"] = 1.0
    elif fam == R.ACC:
        hdr["amax"] = 2.0
    elif fam == R.COMM_PAIR:
        hdr["radius"] = 0.5 * cls.comm_range - near
    elif fam == R.COMM_WAYPOINT:
        hdr["next_waypoint"][ax] = hover[ax] + (0.5 * cls.comm_range - near) * (-1.0 if side == 0 else 1.0)
    names, _ = R.model(cls, hdr, rows, sfc if cls.use_sfc else None)
    X = x.reshape(cls.dim, cls.M, 6)
    (target,) = [e for e in names if e[:5] == (fam, obs, seg, pt, ax)]
    trow = target[5][side if len(target[5]) == 2 else 0]
    eqs = [e for e in names if e[0] == R.EQUALITY]
    Aeq = np.array([_dense(e[5][0], cls) for e in eqs])
    nv = Aeq.shape[1]
    if fam == R.EQUALITY:
        c = np.array([(by if side == 0 else -by) if e is target else 0.0 for e in eqs])
        return hdr, rows, sfc, x + np.linalg.lstsq(Aeq, c, rcond=None)[0]
    v0, _ = R.evaluate(trow, X)
    a_t = _dense(trow, cls)
    want = (by - v0) * (1.0 if trow.sense == "<=" else -1.0)
    B = np.array([_dense(e[5][0], cls) for e in names if e[0] == fam and e is not target] or [np.zeros(nv)])
    H = B.T @ B + 1e-4 * np.eye(nv)
    Cn = np.vstack([Aeq, a_t])
    K = np.block([[H, Cn.T], [Cn, np.zeros((len(Cn), len(Cn)))]])
    rhs = np.concatenate([np.zeros(nv + len(Aeq)), [want]])
    return hdr, rows, sfc, x + np.linalg.solve(K, rhs)[:nv]


def pushed_batch(spec, names, seed=3, world=None):
    """One instance per name in `names`, each with that row pushed.  -> cls, hdr, rows (n, n_obs, M, 6), off, sfc (n, M), x (n, nv); the
    class's world box is `world`, or wide_world(spec)."""
    A = api()
    cls = ref_class(spec, world or wide_world(spec))
    g = np.random.default_rng(seed)
    parts = [pushed_instance(spec, cls, name, g) for name in names]
    hdr = np.array([p[0] for p in parts], A.HEADER_DTYPE)
    rows = np.array([p[1] for p in parts], A.ROW_DTYPE).reshape(len(names), spec[5], spec[0], 6)
    sfc = np.array([p[2] for p in parts], A.BOX_DTYPE)
    x = np.array([p[3] for p in parts])
    return cls, hdr, rows, offsets([spec[5]] * len(names), spec[0]), sfc, x
