"""Constructed inputs for the kernels that run around the QP in every replan -- the goal LP (csrc/lscgoal.hip) and the post-solve
epilogue (csrc/lscpost.hip) -- and plain numpy restatements of what the reference computes there.  No QP is solved anywhere: every case
states its expected result by construction, tests/test_goal.py and tests/test_post.py hold the CPU oracle to it without a device and the
kernels to both on one.

The restatements follow the reference's expressions and nothing else: float32 wherever the reference holds a point3d (control points of
desired_traj, states, boxes, obstacle positions, the point3d difference and its norm), fp64 elsewhere, float32 sums without contraction
(numpy rounds every float32 operation).  They know nothing of the kernels' lane layout or of their reciprocal / square-root sequences.

Out of scope: packed rows of a 2-D class with nz != 0.  No producer writes them (the generators zero the z component of a 2-D mission's
normals), so the goal LP's 2-D cases keep nz = 0."""
import math

import numpy as np

DT = 0.2
EPS_FLOAT = 1e-5  # SP_EPSILON_FLOAT
VMAX = np.array([0.7, 1.0, 1.3])  # one limit per axis: a mixed-up axis index cannot pass
AMAX = np.array([2.0, 3.0, 4.0])
BASE = np.array([0.25, -0.5, 0.125])  # float32-representable, inside the +-1 m box


def f32(a):
    """The float32 rounding of `a`, as fp64."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def quantize(v, bits):
    """v rounded to `bits` significant bits: small multiples of it (and of 25, 500) stay exact in float32."""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


# ---- plan families: x4[n][dim][M][6] -------------------------------------------------------------------------------------------
def const_plan(points, M, dim):
    """Every control point of agent q equals points[q]: the position is exact at every time."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.repeat(np.repeat(points[:, :dim, None, None], M, axis=2), 6, axis=3).copy()


def piecewise_plan(points, M, dim):
    """points[n][M][3]: segment m holds points[q, m] in all six control points (exact positions, and the segment search is exercised)."""
    points = np.asarray(points, dtype=np.float64)
    return np.repeat(np.transpose(points[:, :, :dim], (0, 2, 1))[:, :, :, None], 6, axis=3).copy()


def set_linear(x4, q, m, k, p, h):
    """c_i = p + i h: constant velocity 5 h / dt."""
    x4[q, k, m, :] = p + np.arange(6) * h


def set_quadratic(x4, q, m, k, p, a):
    """c_i = p + i^2 a / 2: first differences (2 i + 1) a / 2, second differences a -> constant acceleration 5 * 4 * a / dt^2."""
    x4[q, k, m, :] = p + np.arange(6) ** 2 * (a / 2)


def linear_velocity(h, dt=DT):
    return 5.0 * h / dt


def quadratic_acceleration(a, dt=DT):
    return 20.0 * a / (dt * dt)


def quadratic_velocity(a, tn, dt=DT):
    """velocity of set_quadratic's segment at normalised time tn: control points 5 (2 i + 1) a / (2 dt), linear in i."""
    return 5.0 * a / (2 * dt) * (1 + 8 * tn)


def flat(x4):
    return np.ascontiguousarray(x4.reshape(x4.shape[0], -1))


# ---- restatements ---------------------------------------------------------------------------------------------------------------
def segment_of(M, dt, t):
    """Trajectory::getPointAt's segment search (reference src/trajectory.cpp:121-136): (segment, normalised time)."""
    end = 0.0
    for idx in range(M):
        end += dt
        if t < end:
            return idx, 1 - (end - t) / dt
    return M - 1, 1.0


def _bern(cp, n, t):
    s = np.zeros(cp.shape[:-1])
    for i in range(n + 1):
        s = s + cp[..., i] * math.comb(n, i) * math.pow(t, i) * math.pow(1 - t, n - i)
    return s


def state_at_np(x4, dt, t, z_2d):
    """Trajectory::getStateAt on float32 control points (desired_traj), as State holds it: (pos, vel, acc)[n][3], float32 values; a 2-D
    mission's z is world_z_2d and its z velocity / acceleration 0 (AgentManager::doStep)."""
    n, dim, M, _ = x4.shape
    m, tn = segment_of(M, dt, t)
    c = f32(x4[:, :, m, :])
    d1 = (c[..., 1:] - c[..., :-1]) * (5 / dt)
    d2 = (d1[..., 1:] - d1[..., :-1]) * (4 / dt)
    out = [np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))]
    out[0][:, :dim], out[1][:, :dim], out[2][:, :dim] = f32(_bern(c, 5, tn)), f32(_bern(d1, 4, tn)), f32(_bern(d2, 3, tn))
    if dim == 2:
        out[0][:, 2] = f32(z_2d)
    return out


def validate_step_np(x4, vmax, amax, bmin, bmax, dt, time_step, z_2d):
    """TrajPlanner::isSolValid (reference src/traj_planner.cpp:990-1045) + doStep's state: (valid[n], state[n][9]).  bmin / bmax [n][M][3]
    or None (no corridors).  Box::isPointInBox is strict with SP_EPSILON_FLOAT on float32 bounds; segment 0 is judged from control point 3."""
    n, dim, M, _ = x4.shape
    ok = np.ones(n, dtype=bool)
    if bmin is not None:
        c = np.empty((n, 3, M, 6))
        c[:, :dim] = f32(x4)
        c[:, dim:] = f32(z_2d)
        lo, hi = f32(bmin).transpose(0, 2, 1)[..., None] - EPS_FLOAT, f32(bmax).transpose(0, 2, 1)[..., None] + EPS_FLOAT
        inside = (c > lo) & (c < hi)
        inside[:, :, 0, :3] = True
        ok &= inside.all(axis=(1, 2, 3))
    pos, vel, acc = state_at_np(x4, dt, time_step, z_2d)
    for k in range(dim):
        ok &= ~(np.abs(vel[:, k]) > vmax[:, k] * 1.01) & ~(np.abs(acc[:, k]) > amax[:, k] * 1.01)
    return ok.astype(np.int32), np.concatenate([pos, vel, acc], axis=1)


def safety_metrics_np(x4_all, radius, downwash, vmax, amax, first, n_loc, n_samples, step, dt, z_2d, lo=0, hi=None):
    """MultiSyncSimulator::update's agent-agent figures (reference src/multi_sync_simulator.cpp:486-577) for the local agents
    [first, first + n_loc) against the agents [lo, hi): [n_loc][9] = ratio, closest agent, sample, vel excess[3], acc excess[3].
    The first strict minimum in (sample, j) order; +inf, -1, -1 without another agent; the excess ratios are signed and kept where
    positive.  vmax / amax: [n_loc][3]."""
    n_total, dim = x4_all.shape[:2]
    hi = n_total if hi is None else hi
    out = np.zeros((n_loc, 9))
    out[:, 0], out[:, 1], out[:, 2] = np.inf, -1, -1
    loc = np.arange(first, first + n_loc)
    others = np.arange(lo, hi)
    rs = radius[loc, None] + radius[None, others]
    dwn = (downwash[loc] * radius[loc])[:, None] + (downwash[others] * radius[others])[None, :]
    dwn = dwn / rs
    for s in range(n_samples):
        pos, vel, acc = state_at_np(x4_all, dt, s * step, z_2d)
        for k in range(dim):
            ve, ae = (vel[loc, k] - vmax[:, k]) / vmax[:, k], (acc[loc, k] - amax[:, k]) / amax[:, k]
            out[:, 3 + k] = np.where((ve > 0) & (ve > out[:, 3 + k]), ve, out[:, 3 + k])
            out[:, 6 + k] = np.where((ae > 0) & (ae > out[:, 6 + k]), ae, out[:, 6 + k])
        if len(others) == 0:
            continue
        p = pos.astype(np.float32)
        dx, dy = p[loc, None, 0] - p[None, others, 0], p[loc, None, 1] - p[None, others, 1]
        dz = ((p[loc, None, 2] - p[None, others, 2]).astype(np.float64) / dwn).astype(np.float32)
        nsq = (dx * dx + dy * dy) + dz * dz  # float32, every operation rounded
        ratio = np.sqrt(nsq.astype(np.float64)) / rs
        ratio[loc[:, None] == others[None, :]] = np.inf
        j = np.argmin(ratio, axis=1)  # the first j attaining the sample's minimum
        r = ratio[np.arange(n_loc), j]
        take = r < out[:, 0]
        out[take, 0], out[take, 1], out[take, 2] = r[take], others[j[take]], s
    return out


def safety_obstacles_np(x4_all, radius, downwash, obs_pos, obs_radius, obs_downwash, skip, first, n_loc, n_samples, step, dt, z_2d):
    """The obstacle leg (reference src/multi_sync_simulator.cpp:527-557): [n_loc][3] = ratio, obstacle, sample; the first strict minimum in
    (sample, obstacle) order, "real" obstacles skipped."""
    out = np.zeros((n_loc, 3))
    out[:, 0], out[:, 1], out[:, 2] = np.inf, -1, -1
    loc = np.arange(first, first + n_loc)
    po = np.asarray(obs_pos, dtype=np.float64).astype(np.float32)
    for s in range(n_samples):
        p = state_at_np(x4_all, dt, s * step, z_2d)[0].astype(np.float32)[loc]
        for o in range(len(po)):
            if skip[o]:
                continue
            dwn = (obs_radius[o] * obs_downwash[o] + radius[loc] * downwash[loc]) / (radius[loc] + obs_radius[o])
            dx, dy = p[:, 0] - po[o, 0], p[:, 1] - po[o, 1]
            dz = ((p[:, 2] - po[o, 2]).astype(np.float64) / dwn).astype(np.float32)
            nsq = (dx * dx + dy * dy) + dz * dz
            ratio = np.sqrt(nsq.astype(np.float64)) / (radius[loc] + obs_radius[o])
            take = ratio < out[:, 0]
            out[take, 0], out[take, 1], out[take, 2] = ratio[take], o, s
    return out


def terminal_segments_np(goal, p0, nominal_velocity, M, dt):
    """getTerminalSegments_old (reference src/traj_optimizer.cpp:530-538): the point3d difference and its norm in float32."""
    d = np.float32(goal).astype(np.float32) - np.asarray(p0, dtype=np.float64).astype(np.float32)
    nsq = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    ts = int((M * dt - math.sqrt(float(nsq)) / nominal_velocity + 1e-9) / dt)
    return max(ts, 1)


# ---- A. goal LP -------------------------------------------------------------------------------------------------------------------
GOAL_M = 5
W3 = np.array([0.3, -0.2, 1.0])
DGW3 = np.array([1.4, -1.1, -0.4])  # signs chosen so that face 0 and the last face of the box can hold the binding LOWER bound
FAR = 10.0


def _dgw(dim):
    d = DGW3.copy()
    if dim == 2:
        d[2] = 0.0
    return d


def row_through(nrm, w, dgw, t):
    """The packed row n . c >= b whose boundary passes through w + dgw t: a lower bound on t if n . dgw > 0, an upper one if < 0."""
    nrm = np.asarray(nrm, dtype=np.float64)
    return np.r_[nrm, nrm @ (w + dgw * t)]


def _normal(rng, dim, dgw, sign):
    """A random normal (length 0.5 .. 2) with sign * n . dgw >= 0.1."""
    while True:
        n = rng.normal(size=3)
        if dim == 2:
            n[2] = 0.0
        n *= rng.uniform(0.5, 2.0) / np.linalg.norm(n)
        if sign * (n @ dgw) >= 0.1:
            return n


def _filler(rng, dim, w, dgw, count):
    """Rows that bind nothing: lower bounds at t <= 0.3, upper bounds behind the variable's cap."""
    rows = np.zeros((count, 4))
    for r in range(count):
        if rng.random() < 0.5:
            rows[r] = row_through(_normal(rng, dim, dgw, +1), w, dgw, rng.uniform(-0.5, 0.3))
        else:
            rows[r] = row_through(_normal(rng, dim, dgw, -1), w, dgw, rng.uniform(1.2, 2.0))
    return rows


def goal_agent(dim, rows, kind, t=None, bind=None, w=None, dgw=None, box=None, p0=None, nominal_velocity=1.0, name=""):
    """kind: "t" (OPTIMAL, goal = w + dgw t; bind = the obstacle row that holds t, whose stored values decide it to the last bit),
    "infeasible" (goal keeps its bits), "waypoint" (|g - w| < SP_EPSILON_FLOAT: goal = w)."""
    w = W3.copy() if w is None else np.asarray(w, dtype=np.float64)
    dgw = _dgw(dim) if dgw is None else np.asarray(dgw, dtype=np.float64)
    box = (np.full(3, -FAR), np.full(3, FAR)) if box is None else box
    return dict(dim=dim, rows=np.asarray(rows, dtype=np.float64).reshape(-1, 4), kind=kind, t=t, bind=bind, w=w, goal=w + dgw, box=box,
                p0=w.copy() if p0 is None else np.asarray(p0, dtype=np.float64), nominal_velocity=nominal_velocity, name=name)


def rows_in_format(rows, fmt):
    return f32(rows) if fmt == "f32" else rows


def expected_t(ag, fmt):
    """The t the LP must return, from the binding row AS STORED in the row format (a face or a bound of the variable: the nominal t)."""
    if ag["bind"] is None:
        return ag["t"]
    r = rows_in_format(ag["rows"], fmt)[ag["bind"]]
    dgw, dim = ag["goal"] - ag["w"], ag["dim"]
    a, c = r[:dim] @ dgw[:dim], r[:dim] @ ag["w"][:dim] - r[3]
    return -c / a


def goal_rowcount_agents(dim, use_sfc, seed=0):
    """Row counts around the 64-lane stride of the row loop: the binding lower bound at row index 0, 63, 64 and last (faces first, then
    obstacles, the order of the kernel's loop and of the reference's model), and a binding UPPER bound at an index >= 64 (infeasible)."""
    rng = np.random.default_rng(1000 * dim + 10 * int(use_sfc) + seed)
    w, dgw = W3, _dgw(dim)
    nf = 2 * dim if use_sfc else 0
    out = []
    for n_obs in ([0, 58, 59, 64, 65, 150] if use_sfc else [63, 64, 65, 129]):
        total = nf + n_obs
        for pos in sorted({0, 63, 64, total - 1}):
            if pos >= total:
                continue
            rows = _filler(rng, dim, w, dgw, n_obs)
            lo, hi = np.full(3, -FAR), np.full(3, FAR)
            bind = None
            if pos < nf:  # a face: even = +e_k . c >= bmin_k, odd = -e_k . c >= -bmax_k
                k = pos >> 1
                assert (dgw[k] > 0) == (pos % 2 == 0)
                (lo if pos % 2 == 0 else hi)[k] = w[k] + dgw[k] * 0.5
            else:
                bind = pos - nf
                rows[bind] = row_through(_normal(rng, dim, dgw, +1), w, dgw, 0.5)
            out.append(goal_agent(dim, rows, "t", t=0.5, bind=bind, box=(lo, hi), name="rows%d_bind%d" % (total, pos)))
        for pos in sorted({64, total - 1}):
            if pos < 64 or pos < nf + 1 or pos >= total:
                continue
            rows = _filler(rng, dim, w, dgw, n_obs)
            rows[0] = row_through(_normal(rng, dim, dgw, +1), w, dgw, 0.5)
            rows[pos - nf] = row_through(_normal(rng, dim, dgw, -1), w, dgw, 0.2)  # t <= 0.2 against t >= 0.5
            out.append(goal_agent(dim, rows, "infeasible", name="rows%d_upper%d" % (total, pos)))
    return out


def goal_edge_agents(dim):
    """a == 0 rows, the short-normal skip, the variable's cap and the |g - w| threshold, on an axis-aligned g - w."""
    w, d = np.array([0.0, 0.0, 1.0]), np.array([2.0, 0.0, 0.0])
    kw = dict(w=w, dgw=d)
    low = lambda t: np.r_[1.0, 0.0, 0.0, 2.0 * t]  # noqa: E731  t >= t
    out = []
    # the normal exactly perpendicular to g - w: a feasibility condition c >= 0 on its own
    out.append(goal_agent(dim, [low(0.25), [0, 1, 0, -1e-3]], "t", t=0.25, bind=0, name="a0_feasible", **kw))
    out.append(goal_agent(dim, [low(0.25), [0, 1, 0, 1e-6]], "infeasible", name="a0_infeasible", **kw))
    # t <= 0.1 against t >= 0.5, the same half-space at two lengths of its normal
    for s, kind in ((0.5e-5, "t"), (2e-5, "infeasible")):
        out.append(goal_agent(dim, [low(0.5), np.r_[-1.0, 0.0, 0.0, -0.2] * s], kind, t=0.5, bind=0, name="normal_%g" % s, **kw))
    # the variable's upper bound 1 + SP_EPSILON_FLOAT
    for t in (0.5, 1.0, 1 + 0.5e-5):
        out.append(goal_agent(dim, [low(t)], "t", t=t, bind=0, name="cap_%r" % t, **kw))
    out.append(goal_agent(dim, [low(1 + 1e-4)], "infeasible", name="cap_over", **kw))
    # |g - w| against SP_EPSILON_FLOAT: below it the LP does not run (the rows would make it infeasible)
    out.append(goal_agent(dim, [low(0.5), [-1, 0, 0, -0.1e-5]], "waypoint", w=w, dgw=[0.5e-5, 0, 0], name="gw_short"))
    out.append(goal_agent(dim, [np.r_[1.0, 0.0, 0.0, 1e-5]], "t", t=0.5, bind=0, w=w, dgw=[2e-5, 0, 0], name="gw_long"))
    # no row at all: t = 0
    out.append(goal_agent(dim, np.zeros((0, 4)), "t", t=0.0, name="no_rows", **kw))
    return out


def goal_ragged_agents(dim, use_sfc):
    """Nine different agents with ragged row counts, zero-row agents included, for the batch tails n = 1, 3, 4, 5, 9."""
    rc = [a for a in goal_rowcount_agents(dim, use_sfc, seed=7)]
    ed = goal_edge_agents(dim)
    pick = [ed[-1], rc[0], ed[1], rc[-1], ed[0], rc[len(rc) // 2], ed[-1], ed[4], rc[3]]
    return pick


def goal_fin_agents(dim, M=GOAL_M, dt=DT):
    """Finished headers: |new goal - p0| = nominal_velocity dt j +- 1e-3 m for j = 0 .. M + 1 puts both sides of every integer step of
    terminal_segments, its floor at 1 included.  Returns (agents, terminal_segments expected by construction); two agents are infeasible
    and are finished from their OLD goal."""
    w, dgw = W3, _dgw(dim)
    out, want = [], []
    rng = np.random.default_rng(40 + dim)
    for j in range(M + 2):
        for sgn in (+1, -1):
            nv = (1.0, 0.8)[j % 2]
            dist = abs(nv * dt * j + sgn * 1e-3)
            for kind in (("t", "infeasible") if j in (2, 4) and sgn > 0 else ("t",)):
                rows = _filler(rng, dim, w, dgw, 5)
                rows[2] = row_through(_normal(rng, dim, dgw, +1), w, dgw, 0.5)
                if kind == "infeasible":
                    rows[4] = row_through(_normal(rng, dim, dgw, -1), w, dgw, 0.2)
                end = w + dgw * (0.5 if kind == "t" else 1.0)  # where the goal ends up: the LP's point, or the old goal
                out.append(goal_agent(dim, rows, kind, t=0.5, bind=2, p0=end - np.array([dist, 0, 0]), nominal_velocity=nv,
                                      name="fin_j%d%+d_%s" % (j, sgn, kind)))
                # (M dt - dist / nv) / dt = M - j -+ 1e-3 / (nv dt); j = 0 has dist = 1e-3 on both sides
                want.append(max(1, M - j - 1 if (sgn > 0 or j == 0) else M - j))
    return out, np.array(want)


# ---- B. isSolValid and doStep ---------------------------------------------------------------------------------------------------
def validate_groups(M, dim, dt=DT):
    """Groups of cases that share one launch: dict(name, time_step, z_2d, x4, vmax, amax, bmin, bmax, valid, names).  `valid` is the verdict
    by construction."""
    z0 = float(BASE[2])
    groups = []

    def group(name, time_step, cases, z_2d=z0):
        n = len(cases)
        x4 = np.stack([c["x"] for c in cases])
        bmin = np.stack([c.get("bmin", np.full((M, 3), -1.0)) for c in cases])
        bmax = np.stack([c.get("bmax", np.full((M, 3), 1.0)) for c in cases])
        vmax = np.stack([c.get("vmax", VMAX) for c in cases]).astype(np.float64)
        amax = np.stack([c.get("amax", AMAX) for c in cases]).astype(np.float64)
        groups.append(dict(name=name, time_step=time_step, z_2d=z_2d, x4=x4, vmax=vmax, amax=amax, bmin=bmin, bmax=bmax,
                           valid=np.array([c["valid"] for c in cases], dtype=np.int32), names=[c["name"] for c in cases], n=n))

    base = lambda: const_plan(BASE[None], M, dim)[0]  # noqa: E731

    # box margin: strict, SP_EPSILON_FLOAT wide, float32 bounds.  A moved point changes its segment's state, so the step is taken elsewhere.
    points = [(0, 3), (1, 0), (M - 1, 5)] + ([(10, 4), (11, 5)] if M == 12 else [])
    for seg0, time_step in ((True, 1.5 * dt), (False, 0.5 * dt)):
        cases = []
        for (m, i) in points:
            if (m == 0) != seg0:
                continue
            for k in range(dim):
                for side in (+1, -1):
                    for delta, valid in ((0.5e-5, 1), (2e-5, 0)):
                        x = base()
                        x[k, m, i] = side * (1.0 + delta)
                        cases.append(dict(x=x, valid=valid, name="box_m%d_i%d_k%d_%+d_%g" % (m, i, k, side, delta)))
        if not seg0:
            # a 30 m box, where a float32 ulp is 1.9e-6 m ...
            for side in (+1, -1):
                for delta, valid in ((0.5e-5, 1), (2e-5, 0)):
                    x = base()
                    x[0, 1, 2] = side * (30.0 + delta)
                    cases.append(dict(x=x, valid=valid, bmin=np.full((M, 3), -30.0), bmax=np.full((M, 3), 30.0), name="box30_%+d_%g" % (side, delta)))
            # ... and a bound that float32 does not hold: 30.000001 is kept as 30 + 2^-19, so 30 + 6 * 2^-19 = 30.00001144 is inside the
            # margin of the float32 bound (30.0000119) and outside that of the fp64 one (30.000011); one float32 step further it is outside both
            for steps, valid in ((6, 1), (7, 0)):
                x = base()
                x[1, 2, 4] = 30.0 + steps * 2.0 ** -19
                bmax = np.full((M, 3), 40.0)
                bmax[2, 1] = 30.000001
                cases.append(dict(x=x, valid=valid, bmin=np.full((M, 3), -40.0), bmax=bmax, name="box_unrepresentable_%d" % steps))
        group("box_seg0" if seg0 else "box", time_step, cases)

    # (m = 0, i < 3) is never judged: 1 m outside, alone and together (the step is taken in segment 1: segment 0's state is wild)
    cases = []
    for which in ([0], [1], [2], [0, 1, 2]):
        x = base()
        for i in which:
            x[:, 0, i] = 2.0
        cases.append(dict(x=x, valid=1, name="skipped_%s" % which))
    x = base()
    x[0, 0, 3] = 2.0
    cases.append(dict(x=x, valid=0, name="not_skipped_3"))
    group("skipped", 1.5 * dt, cases)

    # dynamic limits, 1 % tolerance, one limit per axis; evaluated in the middle of segment 0
    cases = []
    for k in range(dim):
        for sgn in (+1, -1):
            for f, valid in ((1.0099, 1), (1.0101, 0)):
                x = base()
                set_linear(x[None], 0, 0, k, 0.0, sgn * f * VMAX[k] * dt / 5)
                cases.append(dict(x=x, valid=valid, name="vel_k%d_%+d_%g" % (k, sgn, f)))
                x = base()
                a = sgn * f * AMAX[k] * dt * dt / 20
                assert abs(quadratic_velocity(a, 0.5, dt)) < 0.9 * VMAX[k]  # the velocity it implies stays inside its limit
                set_quadratic(x[None], 0, 0, k, 0.0, a)
                cases.append(dict(x=x, valid=valid, name="acc_k%d_%+d_%g" % (k, sgn, f)))
    group("limits", 0.5 * dt, cases)

    # times: inside a segment, on a boundary, behind the horizon (the ms < 0 branch); a piecewise-constant plan and one with linear segments
    pts = np.zeros((1, M, 3))
    pts[0] = BASE + np.arange(M)[:, None] * np.array([0.03125, -0.015625, 0.0625])
    if dim == 2:
        pts[0, :, 2] = z0
    for time_step in (0.5 * dt, dt, 2.5 * dt, M * dt, M * dt + 1):
        pw = piecewise_plan(pts, M, dim)[0]
        lin = pw.copy()
        for k in range(dim):
            set_linear(lin[None], 0, 2, k, pts[0, 2, k], 0.5 * VMAX[k] * dt / 5)
            set_linear(lin[None], 0, M - 1, k, pts[0, M - 1, k], -0.4 * VMAX[k] * dt / 5)
        group("time_%g" % time_step, time_step, [dict(x=pw, valid=1, name="piecewise"),
                                                 dict(x=lin, valid=1, name="linear")])
        groups[-1]["piecewise_point"] = pts[0, segment_of(M, dt, time_step)[0]]

    if dim == 2:
        # world_z_2d against the box's z range; the limits of the z axis are never judged (a negative one would fail any velocity)
        for off, valid in ((2e-5, 0), (0.5e-5, 1), (-0.5e-5, 1)):
            for side in (+1, -1):
                group("z2d_%+d_%g" % (side, off), 0.5 * dt,
                      [dict(x=base(), valid=valid, vmax=np.array([0.7, 1.0, -1.0]), amax=np.array([2.0, 3.0, -1.0]), name="z2d")],
                      z_2d=side * (1.0 + off))
    return groups


def commit_case(M, dim, api):
    """The chain's commit: seven agents, every status; x_new of a failed agent and x_init of a solved one are NaN.  Agent 5 (OPTIMAL) is
    out of its box, agent 3 (NUMERIC) falls back on an initial trajectory that is too fast, agent 1's (INFEASIBLE) fallback is valid."""
    status = np.array([api.STATUS_OPTIMAL, api.STATUS_INFEASIBLE, api.STATUS_ITER_LIMIT, api.STATUS_NUMERIC, api.STATUS_CAPACITY,
                       api.STATUS_OPTIMAL, api.STATUS_OPTIMAL], dtype=np.int32)
    n = len(status)
    pts = BASE + np.arange(n)[:, None] * np.array([0.015625, 0.03125, -0.0078125])
    x_new, x_init = const_plan(pts, M, dim), const_plan(pts + 0.0625, M, dim)
    x_new[5, 1, M - 1, 4] = 1.0 + 2e-5
    set_linear(x_init, 3, 0, 0, 0.0, 1.5 * VMAX[0] * DT / 5)
    chosen = np.where((status == api.STATUS_OPTIMAL)[:, None, None, None], x_new, x_init)
    x_new[status != api.STATUS_OPTIMAL] = np.nan
    x_init[status == api.STATUS_OPTIMAL] = np.nan
    goal = pts[::-1] * 3 + 0.1  # what hdr.goal holds, agent by agent different
    return dict(status=status, x_new=x_new, x_init=x_init, chosen=chosen, goal=goal, valid=np.array([1, 1, 1, 0, 1, 0, 1], dtype=np.int32), n=n)


# ---- C. agent-agent safety figures ------------------------------------------------------------------------------------------------
SAF_M, SAF_RADIUS = 5, 0.15
SAF_STEP, SAF_SAMPLES = DT / 2, 2 * SAF_M + 2  # samples on every segment boundary and behind the horizon


def lattice(n, perm=None, late=False):
    """x_j = j metres on a line, x_{n-1} = n - 1.5; piecewise-constant plans whose third segment doubles the spacing (late: the spacing is
    1 m everywhere and HALVES in segment 3 only, so the minimum is first reached at the first sample inside it).  perm: id perm[j] flies
    lattice place j.  Returns (x4, expected [n][3] = ratio, closest, sample by construction)."""
    place = np.arange(n, dtype=np.float64)
    place[n - 1] = n - 1.5
    scale = np.ones(SAF_M)
    scale[3 if late else 2] = 0.5 if late else 2.0
    pts = np.zeros((n, SAF_M, 3))
    pts[:, :, 0] = place[:, None] * scale[None, :]
    pts[:, :, 1], pts[:, :, 2] = -0.5, 1.0
    ids = np.arange(n) if perm is None else np.asarray(perm)
    x4 = np.zeros((n, 3, SAF_M, 6))
    x4[ids] = piecewise_plan(pts, SAF_M, 3)
    sample = 0
    if late:  # the first sample whose time is not before segment 3 (the segment search's own accumulated sum)
        end = DT + DT + DT
        sample = next(s for s in range(SAF_SAMPLES) if not s * SAF_STEP < end)
    want = np.zeros((n, 3))
    shrink = 0.5 if late else 1.0
    for j in range(n):
        if n == 1:
            want[ids[j]] = np.inf, -1, -1
            continue
        nb = [(abs(place[j] - place[o]), ids[o]) for o in (j - 1, j + 1) if 0 <= o < n]
        d = min(nb)[0]
        want[ids[j]] = d * shrink / (2 * SAF_RADIUS), min(i for dd, i in nb if dd == d), sample  # a tie goes to the lower id
    return x4, want


def scattered(n, seed):
    """Seeded float32 positions (piecewise constant, so exact on both sides) in a 6 m cube: no lattice, no exact square roots."""
    rng = np.random.default_rng(seed)
    pts = f32(rng.uniform(0.0, 6.0, (n, SAF_M, 3)))
    return piecewise_plan(pts, SAF_M, 3)


def excess_case():
    """One agent per (axis, factor): linear plans with v_k in {1.5, -2, 0.99} vmax_k and quadratic ones for amax_k, 20 m apart.  The
    step h is cut to 19 bits (a to 15), so that every control point, 25 h and 500 a are exact in float32 and the velocity / acceleration is
    the same float32 value at every time; the 1.5 agents get the limit V / 1.5, which makes the ratio 0.5 up to fp64 rounding.
    Returns (x4, vmax[n][3], amax[n][3], want_vel[n][3], want_acc[n][3]); the signed ratio of -2 vmax is -3: no excess."""
    cases = [(kind, k, f) for kind in "va" for k in range(3) for f in (1.5, -2.0, 0.99)]
    n = len(cases)
    pts = np.zeros((n, 3))
    for q, (_, k, _) in enumerate(cases):
        pts[q, (k + 1) % 3] = 20.0 * q  # (apart along an axis that does not move: the moving one starts at 0 and stays exact)
    x4 = const_plan(pts, SAF_M, 3)
    vmax, amax = np.tile(VMAX, (n, 1)), np.tile(AMAX, (n, 1))
    want_v, want_a = np.zeros((n, 3)), np.zeros((n, 3))
    for q, (kind, k, f) in enumerate(cases):
        for m in range(SAF_M):
            if kind == "v":
                h = float(quantize(f * VMAX[k] * DT / 5, 19))
                set_linear(x4, q, m, k, pts[q, k], h)
                if f == 1.5:
                    vmax[q, k] = linear_velocity(h) / 1.5
            else:
                a = float(quantize(f * AMAX[k] * DT * DT / 20, 15))
                set_quadratic(x4, q, m, k, pts[q, k], a)
                vmax[q, k] = 100.0  # (the velocity the segment implies is not what this agent is about)
                if f == 1.5:
                    amax[q, k] = quadratic_acceleration(a) / 1.5
        (want_v if kind == "v" else want_a)[q, k] = 0.5 if f == 1.5 else 0.0
    return x4, vmax, amax, want_v, want_a


MISSION_OFFSETS = [0, 1, 32, 64, 97, 354]  # missions of 1, 31, 32, 33 and 257 agents


def missions_case(seed=9):
    """Scattered agents cut into missions that overlap in space; the last agent of mission 1 and the first of mission 2 hover 0.1 m
    apart (neither may see the other); one agent per mission flies 1.5 vmax, and every agent has limits of its own."""
    n = MISSION_OFFSETS[-1]
    x4 = scattered(n, seed)
    x4[32] = x4[31]
    x4[32, 0] += f32(0.1)
    vmax = VMAX[None] * (1 + np.arange(n)[:, None] / 1024.0)
    amax = AMAX[None] * (1 + np.arange(n)[:, None] / 2048.0)
    for a in (0, 5, 40, 96, 353):
        h = float(quantize(1.5 * VMAX[a % 3] * DT / 5, 19))
        for m in range(SAF_M):
            set_linear(x4, a, m, a % 3, 0.0, h)
    return x4, vmax, amax


# ---- D. obstacle safety figures -----------------------------------------------------------------------------------------------------
def obstacles_case(n_agents, api):
    """Agents on a line (constant plans); obstacles 1 and 3 are twins mirrored in that line -- equal distance, radius and downwash, so the
    lower index must win, exactly -- obstacle 0 wins near x = 0, obstacle 4 nowhere, and the "real" obstacle 2 sits ON the line, nearer
    than all of them, and is never chosen.  Radius * downwash is exact in fp64 for every obstacle and agent."""
    pts = np.zeros((n_agents, 3))
    pts[:, 0] = np.arange(n_agents) * 0.125
    pts[:, 2] = 1.0
    x4 = const_plan(pts, SAF_M, 3)
    obs = np.zeros(5, api.OBSTACLE_DTYPE)
    obs["position"] = [[0.0, 5.0, 1.5], [20.0, 3.0, 0.5], [16.0, 0.0, 1.0], [20.0, -3.0, 0.5], [16.0, 40.0, 1.0]]
    obs["radius"] = [0.5, 0.25, 0.25, 0.25, 0.5]
    obs["downwash"] = [1.5, 2.0, 2.0, 2.0, 1.0]
    obs["max_acc"] = 1.0
    obs["type"][2] = api.OBSTACLE_REAL
    return x4, obs
