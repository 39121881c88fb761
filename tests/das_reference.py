"""A plain numpy restatement of the dual active-set phase (csrc/lscqp_das.hpp, lscqp_das_body.inc) -- CPU only, float64, for the tests.

Goldfarb-Idnani in CONTROL-POINT space, as the kernel runs it (grown from tools/proto_das.py):

    min 1/2 c'Hx c + fx'c   over c = cfix + T z,   rows a'c >= h          (c relative to the agent's position p0)
    C = T (T'Hx T)^-1 T'    the compliance of the plan, per number of terminal segments
    one step for row p      w_p = C a_p;  r = S^-1 A'w_p  (S = A'C A over the active rows);  dc = w_p - W r;
                            t1 = min_{r_j > 0} u_j / r_j (lowest position on ties),  t2 = -slack_p / a_p'dc;
                            t2 <= t1: p joins;  otherwise the row at t1 leaves and the step is repeated for the same p.

What is the KERNEL's and restated here on purpose:
  * row ids  [LSC o*P + cp | interval lo/hi per (axis, cp) | velocity lo/hi | acceleration lo/hi | communication pairs lo/hi]; the two-sided
    families come in pairs nL + 2 r + side (side 0: stencil - lo >= 0, side 1: hi - stencil >= 0);
  * the rows the reference drops (the first three control points; LSC normals with |n|^2 < 1e-10) and the merged interval of one control
    point (world box, or +-100 for z of segment 0 in RSFC; corridor; on c[m][5] the range rows against c[0][0] and the waypoint);
  * the SELECTION RULE: the row with the smallest RAW slack (metres, not divided by the row's norm), lowest id on ties, violated if its
    slack is below -1e-9 (pass_local / `see` in the body: `slack < bv`, threads and wavefronts combined lexicographically on (slack, id));
  * the budgets: a violated row with `kmax` rows already held ends the phase (WHY_ROWS), the step counter counts every partial step --
    the ones that drop a row too -- and ends it when it exceeds `max_steps` (WHY_STEPS).
What is NOT restated: the factor J = L^-1 and its rotations (S is solved afresh each step), the polish (float64 with a fresh solve does not
drift), LDS staging, row formats -- none of them changes which step is taken.

Besides the optimum, `das` reports how clearly every decision was made: the smallest MARGIN, in metres of the candidate's slack, by which a
selection (runner-up row, or the -1e-9 bar) or a ratio test (t1 against t2, t1 against the next row's) was decided.  A row that is the same
row on the plan's subspace as the chosen one (equal C a and equal slack: c[m][5] and c[m+1][0] under one bound, a plane given twice) is no
runner-up: whichever of the two is taken, the step is the same and the other one ends at slack 0.  At the last look a row in the span of
the held rows at zero slack counts as held.  A case whose margin is far above both
sides' rounding must take the same steps on the device; the GPU test compares step counts on those."""
import numpy as np

TOLP = 1e-9
WHY_ROWS, WHY_STEPS, WHY_NO_STEP = 3, 4, 5  # LSCQP_DAS_WHY_* of include/lscqp.h

Q_INT = np.array([[720, -1800, 1200, 0, 0, -120], [-1800, 4800, -3600, 0, 600, 0], [1200, -3600, 3600, -1200, 0, 0],
                  [0, 0, -1200, 3600, -3600, 1200], [0, 600, 0, -3600, 4800, -1800], [-120, 0, 0, 1200, -1800, 720]], dtype=float)
TB = np.array([[0.0, 0.0, 1.0], [0.0, -1.0, 2.0], [1.0, -4.0, 4.0]])


def null_space_map(M, end_stop):
    """c = cfix + T z: the equality rows of the model (initial state, C0/C1/C2 junctions, end stop) eliminated."""
    nza = 3 * (M - 1) + (1 if end_stop else 3)
    T = np.zeros((6 * M, nza))
    for m in range(M):
        last = end_stop and m == M - 1
        for j in range(3):
            T[6 * m + 3 + j, 3 * m + (0 if last else j)] = 1.0
        if m >= 1:
            T[6 * m:6 * m + 3, 3 * (m - 1):3 * (m - 1) + 3] = TB
    return T


_TABLES = {}


def tables(M, end_stop, dt, w_c, w_t, ts):
    key = (M, bool(end_stop), dt, w_c, w_t, ts)
    if key not in _TABLES:
        T = null_space_map(M, end_stop)
        Hx = np.kron(np.eye(M), 2 * w_c * Q_INT * dt ** -5)
        for m in range(M - ts, M):
            Hx[6 * m + 5, 6 * m + 5] += 2 * w_t
        K = T.T @ Hx @ T
        Ki = np.linalg.inv(K)
        Ki = Ki + Ki @ (np.eye(len(K)) - K @ Ki)  # one Newton refinement of the inverse
        C = T @ (0.5 * (Ki + Ki.T)) @ T.T
        _TABLES[key] = (T, Hx, C)
    return _TABLES[key]


def rows_of(M, dim, dt, comm_range, use_sfc, rsfc, wmin, wmax, ag, lsc, sfc):
    """Every row of one instance in the kernel's id order: list of (entries [(axis, cp, coef)], rhs, family, live).
    ag: one record with p0, v0, a0, goal, next_waypoint, vmax, amax, radius; lsc: packed rows (n_obs, M, 6) with nx, ny, nz, b or None;
    sfc: boxes (M) with bmin, bmax or None."""
    P = 6 * M
    org = np.asarray(ag["p0"], float).reshape(3)
    rows = []
    if lsc is not None:
        L = np.asarray(lsc).reshape(-1)
        for j in range(len(L)):
            nx, ny, nz, b = float(L["nx"][j]), float(L["ny"][j]), float(L["nz"][j]), float(L["b"][j])
            cp = j % P
            live = not (nx * nx + ny * ny + nz * nz < 1e-10) and cp >= 3
            n = [nx, ny, nz if dim == 3 else 0.0]
            rhs = b - (nx * org[0] + ny * org[1] + (nz * org[2] if dim == 3 else 0.0))
            rows.append(([(k, cp, n[k]) for k in range(dim)], rhs, "lsc", live))
    rho_pair = 0.5 * comm_range - float(ag["radius"])
    rho_wp = 0.5 * comm_range - 1e-5
    wp = np.asarray(ag["next_waypoint"], float).reshape(3) - org
    for k in range(dim):
        for cp in range(P):
            m = cp // 6
            lo, hi = wmin[k] - org[k], wmax[k] - org[k]
            if rsfc and k == 2 and m == 0:
                lo, hi = -100.0 - org[k], 100.0 - org[k]
            if use_sfc:
                lo, hi = max(lo, float(sfc["bmin"][m][k]) - org[k]), min(hi, float(sfc["bmax"][m][k]) - org[k])
            if comm_range > 0 and cp % 6 == 5:
                lo, hi = max(lo, -rho_pair, wp[k] - rho_wp), min(hi, rho_pair, wp[k] + rho_wp)
            rows.append(([(k, cp, 1.0)], lo, "interval", cp >= 3))
            rows.append(([(k, cp, -1.0)], -hi, "interval", cp >= 3))
    for k in range(dim):
        hv = float(ag["vmax"][k]) * dt * 0.2
        for m in range(M):
            for i in range(5):
                e, live = 6 * m + i, not (m == 0 and i < 2)
                rows.append(([(k, e + 1, 1.0), (k, e, -1.0)], -hv, "velocity", live))
                rows.append(([(k, e + 1, -1.0), (k, e, 1.0)], -hv, "velocity", live))
    for k in range(dim):
        ha = float(ag["amax"][k]) * dt * dt * 0.05
        for m in range(M):
            for i in range(4):
                e, live = 6 * m + i, not (m == 0 and i < 1)
                rows.append(([(k, e + 2, 1.0), (k, e + 1, -2.0), (k, e, 1.0)], -ha, "acceleration", live))
                rows.append(([(k, e + 2, -1.0), (k, e + 1, 2.0), (k, e, -1.0)], -ha, "acceleration", live))
    for k in range(dim):
        for uu in range(1, M):
            for up in range(uu):
                e2, e1 = 6 * uu + 5, 6 * (up + 1)
                rows.append(([(k, e2, 1.0), (k, e1, -1.0)], -rho_pair, "pair", comm_range > 0))
                rows.append(([(k, e2, -1.0), (k, e1, 1.0)], -rho_pair, "pair", comm_range > 0))
    return rows


def das(M, dim, dt, w_c, w_t, comm_range, end_stop, use_sfc, rsfc, wmin, wmax, ag, lsc, sfc, ts, kmax=32, max_steps=96, trace=None):
    """-> dict(status 'optimal' | WHY_*, x (world frame, axis-major like the ABI), active [(id, family, entries, multiplier)], steps, peak,
    left [(position, rows held)], margin)."""
    P, NX = 6 * M, dim * 6 * M
    T, Hx, C = tables(M, end_stop, dt, w_c, w_t, ts)
    org = np.asarray(ag["p0"], float).reshape(3)
    R = rows_of(M, dim, dt, comm_range, use_sfc, rsfc, wmin, wmax, ag, lsc, sfc)
    nR = len(R)
    A = np.zeros((nR, NX))
    h = np.zeros(nR)
    live = np.zeros(nR, bool)
    for i, (ent, rhs, _, on) in enumerate(R):
        for (k, cp, co) in ent:
            A[i, k * P + cp] += co
        h[i], live[i] = rhs, on
    # unconstrained optimum, axis by axis
    c = np.zeros(NX)
    for k in range(dim):
        c1 = float(ag["v0"][k]) * dt * 0.2
        c2 = float(ag["a0"][k]) * dt * dt * 0.05 + 2.0 * c1
        cfix = np.zeros(P)
        cfix[1], cfix[2] = c1, c2
        fx = np.zeros(P)
        for m in range(M - ts, M):
            fx[6 * m + 5] = -2.0 * w_t * (float(ag["goal"][k]) - org[k])
        c[k * P:(k + 1) * P] = cfix - C @ (Hx @ cfix + fx)

    def Cmul(a):  # C couples control points of one axis only
        return np.concatenate([C @ a[k * P:(k + 1) * P] for k in range(dim)])

    act, W, u = [], [], []
    steps = peak = 0
    left = []
    margin, margin_at = np.inf, None
    status = "optimal"

    def note(value, what):
        nonlocal margin, margin_at
        if value < margin:
            margin, margin_at = value, (what, steps)

    while True:
        slack = np.where(live, A @ c - h, np.inf)
        p = int(np.argmin(slack))  # (first minimum: the lowest id)
        best = slack[p]

        def same_row(j, w, s):  # row j is the row with C a = w and slack s, on the plan's subspace
            return abs(slack[j] - s) < 1e-12 and np.abs(Cmul(A[j]) - w).max() <= 1e-12 * np.abs(w).max()

        if not best < -TOLP:
            # the last look: every row that is not held clears the bar by its slack + 1e-9.  The held rows sit at zero slack up to rounding,
            # 1e-9 above the bar by construction, and so does a row whose normal lies in the span of theirs on the plan's subspace (a twin;
            # a velocity row between two held ones across a junction, where continuity makes the three dependent): it is held by implication
            Wm = np.array(W).T if act else np.zeros((NX, 0))

            def implied(j):
                if abs(slack[j]) > 1e-12 or not act:
                    return False
                w = Cmul(A[j])
                return np.abs(Wm @ np.linalg.lstsq(Wm, w, rcond=None)[0] - w).max() <= 1e-9 * np.abs(w).max()

            for j in np.argsort(slack, kind="stable")[:6 * (len(act) + 2)]:
                if not implied(j):
                    note(slack[j] + TOLP, "last look, row %d" % j)
                    break
            break
        note(-TOLP - best, "violation of row %d" % p)
        wp = Cmul(A[p])
        # the runner-up: the most violated row that is not the same row on the plan's subspace
        for j in np.argsort(slack, kind="stable")[:8]:
            if j != p and not same_row(j, wp, best):
                note(slack[j] - best, "rows %d and %d" % (p, j))
                break
        if len(act) >= kmax:
            status = WHY_ROWS
            break
        spp = A[p] @ wp
        up = 0.0
        stop = False
        while True:
            steps += 1
            if steps > max_steps:
                status, stop = WHY_STEPS, True
                break
            kk = len(act)
            sp = A[p] @ c - h[p]
            if kk:
                Aa, Wm = A[act], np.array(W)
                v = Wm @ A[p]
                r = np.linalg.solve(Aa @ Wm.T, v)
                dc = wp - r @ Wm
                curv = spp - v @ r
            else:
                r, dc, curv = np.zeros(0), wp, spp
            t2 = -sp / curv if curv > 1e-12 * spp else np.inf
            cand = sorted((u[j] / r[j], j) for j in range(kk) if r[j] > 0.0)
            t1, l = cand[0] if cand else (np.inf, -1)
            t = min(t1, t2)
            if not np.isfinite(t):
                status, stop = WHY_NO_STEP, True
                break
            if np.isfinite(t1) or np.isfinite(t2):
                if np.isfinite(t1) and np.isfinite(t2):
                    note(abs(t1 - t2) * curv, "join or drop, row %d" % p)
                if t1 < t2 and len(cand) > 1:
                    note((cand[1][0] - t1) * max(curv, 0.0) if np.isfinite(t2) else np.inf, "which row drops, row %d" % p)
            if trace is not None:
                trace.append(dict(step=steps, row=p, family=R[p][2], slack=sp, t1=t1, t2=t2, held=kk, leaves=(l if t2 > t1 else -1)))
            if np.isfinite(t2):
                c = c + t * dc
            u = [max(0.0, u[j] - t * r[j]) for j in range(kk)]
            up += t
            if t2 <= t1:
                act.append(p), W.append(wp), u.append(up)
                peak = max(peak, len(act))
                break
            left.append((l, kk))
            act.pop(l), W.pop(l), u.pop(l)
        if stop:
            break
    x = np.concatenate([c[k * P:(k + 1) * P] + org[k] for k in range(dim)])
    active = [(i, R[i][2], R[i][0], uj) for i, uj in zip(act, u)]
    return dict(status=status, x=x, active=active, steps=steps, peak=peak, left=left, margin=margin, margin_at=margin_at, n_lsc_rows=0 if lsc is None else np.asarray(lsc).size)
