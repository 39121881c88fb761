"""A restatement of the prescreen's question, and a verifier of its certificates -- numpy, scipy (HiGHS) and mpmath, nothing of the kernel's.

The prescreen (include/lscqp.h, csrc/lscqp_prescreen.hip) asks, per FREE control point cp = m*6 + i (cp >= 3), whether the rows that touch
that point alone have a common point.  Those rows, normalised and relative to the agent's position p0:
    the instance's LSC rows at cp that the solver keeps (|n| >= 1e-5; in a 2-D class only the x, y parts exist),  n^.c >= b^ = (b - n.p0) / |n|;
    the faces of the variable's bounds in the row-for-row model oracle.assemble() builds (world box as lb / ub; corridor faces and, on
    c[m][5], the waypoint's communication range as single-variable rows of G),  c_k >= lo_k - p0_k  and  -c_k >= -(hi_k - p0_k).
t*_cp = min over c of max_i (b^_i - n^_i.c), one small LP: < 0 there is a point with that margin, > 0 every point violates a row by that much.

The three fixed control points of segment 0 have no t*: the reference puts no LSC row on them (src/traj_optimizer.cpp:404-406), the model
holds none, and a row violated there says nothing about the QP.  fixed_point_violation() gives the largest violation of the instance's
rows there all the same, for the cases that show the prescreen must NOT fire on it.

Bars (the issue's): t* >= 1e-5 somewhere -> must fire; max t* <= 0.9e-6 -> must not; in between either answer is right.
"""
import mpmath
import numpy as np

MUST_FIRE_BAR, MUST_NOT_BAR, PROOF_BAR = 1e-5, 0.9e-6, 1e-6
FIRE, QUIET, WINDOW = "FIRE", "QUIET", "WINDOW"


class ClassInfo:
    """What the restatement needs of a solver class."""

    def __init__(self, M, dim, world_min, world_max, use_sfc=True, comm_range=3.0):
        self.M, self.dim, self.P, self.comm_range = M, dim, M * 6, comm_range
        self.world_min, self.world_max, self.use_sfc = np.asarray(world_min, float), np.asarray(world_max, float), use_sfc


def interval(ci, hdr1, sfc1, cp):
    """(lo, hi) of control point cp in absolute coordinates over the class's axes: world box, the corridor box of its segment, and on the last
    point of a segment the communication range about the next waypoint (src/traj_optimizer.cpp:492-498) -- the model's single-variable rows."""
    lo, hi = ci.world_min[:ci.dim].copy(), ci.world_max[:ci.dim].copy()
    if ci.use_sfc:
        lo = np.maximum(lo, np.asarray(sfc1["bmin"][cp // 6], float)[:ci.dim])
        hi = np.minimum(hi, np.asarray(sfc1["bmax"][cp // 6], float)[:ci.dim])
    if ci.comm_range > 0 and cp % 6 == 5:
        w, r = np.asarray(hdr1["next_waypoint"], float)[:ci.dim], 0.5 * ci.comm_range - 1e-5
        lo, hi = np.maximum(lo, w - r), np.minimum(hi, w + r)
    return lo, hi


def point_rows(ci, hdr1, rows1, sfc1, cp):
    """The normalised rows of control point cp, relative to p0: (ids, N [k, dim], b [k]); ids as in lscqp_prescreen_cert.row."""
    n_obs = int(hdr1["n_obs"])
    p0 = np.asarray(hdr1["p0"], float)
    ids, N, b = [], [], []
    R = rows1.reshape(n_obs, ci.P)
    for o in range(n_obs):
        n3 = np.array([R["nx"][o, cp], R["ny"][o, cp], R["nz"][o, cp]], float)
        if np.sqrt(n3 @ n3) < 1e-5:
            continue
        n = n3[:ci.dim]
        nn = np.sqrt(n @ n)
        if nn == 0.0:
            continue
        ids.append(o * ci.P + cp), N.append(n / nn), b.append((float(R["b"][o, cp]) - n @ p0[:ci.dim]) / nn)
    lo, hi = interval(ci, hdr1, sfc1, cp)
    for k in range(ci.dim):
        e = np.zeros(ci.dim)
        e[k] = 1.0
        ids.append(-1 - 2 * k), N.append(e), b.append(lo[k] - p0[k])
        ids.append(-1 - (2 * k + 1)), N.append(-e), b.append(-(hi[k] - p0[k]))
    return np.array(ids), np.array(N), np.array(b)


_MEMO = {}


def t_star_cp(ci, hdr1, rows1, sfc1, cp):
    from scipy.optimize import linprog

    _, N, b = point_rows(ci, hdr1, rows1, sfc1, cp)
    key = (N.tobytes(), b.tobytes())
    if key in _MEMO:  # (the families repeat a base instance's untouched control points many times over)
        return _MEMO[key]
    # variables (c, t): b_i - n_i.c <= t
    A = np.hstack([-N, -np.ones((len(b), 1))])
    res = linprog(np.r_[np.zeros(ci.dim), 1.0], A_ub=A, b_ub=-b, bounds=[(None, None)] * (ci.dim + 1), method="highs")
    if res.status != 0:
        raise RuntimeError("prescreen LP: %s" % res.message)
    _MEMO[key] = float(res.x[-1])
    return _MEMO[key]


def t_star_all(ci, hdr1, rows1, sfc1, cps=None):
    """t*_cp for the free control points (or those of `cps`), -inf for the fixed ones: array [P]."""
    out = np.full(ci.P, -np.inf)
    for cp in (range(3, ci.P) if cps is None else cps):
        if cp >= 3:
            out[cp] = t_star_cp(ci, hdr1, rows1, sfc1, cp)
    return out


def fixed_point_violation(ci, hdr1, rows1, dt=0.2):
    """The largest normalised violation of the instance's LSC rows at c0, c1, c2 of segment 0 (rows the solver never reads)."""
    p0, v0, a0 = (np.asarray(hdr1[f], float) for f in ("p0", "v0", "a0"))
    pts = [p0, p0 + v0 * dt / 5, p0 + 2 * v0 * dt / 5 + a0 * dt * dt / 20]
    n_obs = int(hdr1["n_obs"])
    R = rows1.reshape(n_obs, ci.P)
    worst = -np.inf
    for cp in range(3):
        for o in range(n_obs):
            n = np.array([R["nx"][o, cp], R["ny"][o, cp], R["nz"][o, cp]], float)[:ci.dim]
            nn = np.sqrt(n @ n)
            if nn >= 1e-5:
                worst = max(worst, (float(R["b"][o, cp]) - n @ pts[cp][:ci.dim]) / nn)
    return worst


def label_of(t_max):
    return FIRE if t_max >= MUST_FIRE_BAR else QUIET if t_max <= MUST_NOT_BAR else WINDOW


def model_bounds(model, nv):
    """Per-variable (lo, hi) of oracle.assemble()'s model: lb / ub and every single-variable row of G x <= h."""
    lo, hi = np.array(model["lb"], float), np.array(model["ub"], float)
    G, h = model["G"], model["h"]
    for i in range(G.shape[0]):
        ix = np.flatnonzero(G[i])
        if len(ix) == 1:
            j, a = int(ix[0]), float(G[i, ix[0]])
            if a > 0:
                hi[j] = min(hi[j], h[i] / a)
            else:
                lo[j] = max(lo[j], h[i] / a)
    return lo, hi


class CertError(AssertionError):
    pass


def verify_cert(ci, hdr1, rows1, model, cert, dps=40):
    """Holds one FIRED certificate to its contract in `dps`-digit arithmetic; raises CertError naming what is wrong, returns the recomputed
    proven violation.  rows1: the instance's rows as the device read them (float64 values; f32 rows widened).  model: oracle.assemble()'s."""
    F = mpmath.mpf
    old = mpmath.mp.dps
    mpmath.mp.dps = dps
    try:
        if int(cert["fired"]) != 1:
            raise CertError("not fired")
        cp, k = int(cert["control_point"]), int(cert["n_rows"])
        n_obs = int(hdr1["n_obs"])
        if not (3 <= cp < ci.P):
            raise CertError("control point %d is not a free one" % cp)
        if not (1 <= k <= ci.dim + 1):
            raise CertError("n_rows %d" % k)
        lam = [F(float(x)) for x in cert["lambda"][:k]]
        if any(x < 0 for x in lam):
            raise CertError("negative lambda")
        if abs(mpmath.fsum(lam) - 1) > F(10) ** -12:
            raise CertError("sum lambda = %s" % mpmath.nstr(mpmath.fsum(lam), 17))
        p0 = [F(float(x)) for x in hdr1["p0"]]
        mlo, mhi = model_bounds(model, ci.dim * ci.P)
        rho = [F(0)] * ci.dim
        v = F(0)
        seen = set()
        for j in range(k):
            rid = int(cert["row"][j])
            if rid in seen:
                raise CertError("row %d twice" % rid)
            seen.add(rid)
            if rid >= 0:
                if rid >= n_obs * ci.P or rid % ci.P != cp:
                    raise CertError("row id %d is not a row of control point %d" % (rid, cp))
                n3 = [F(float(rows1[f][rid])) for f in ("nx", "ny", "nz")]
                if mpmath.sqrt(mpmath.fsum(a * a for a in n3)) < F("1e-5"):
                    raise CertError("row %d is one the solver drops" % rid)
                n = n3[:ci.dim]
                nn = mpmath.sqrt(mpmath.fsum(a * a for a in n))
                if nn == 0:
                    raise CertError("row %d has no part in the class's axes" % rid)
                b = (F(float(rows1["b"][rid])) - mpmath.fsum(a * c for a, c in zip(n, p0))) / nn
                n = [a / nn for a in n]
            else:
                f = -1 - rid
                axis, side = f >> 1, f & 1
                if axis >= ci.dim:
                    raise CertError("face id %d: axis %d" % (rid, axis))
                var = axis * ci.P + cp
                bound = mhi[var] if side else mlo[var]
                if not np.isfinite(bound):
                    raise CertError("face id %d: the model does not bound that variable" % rid)
                n = [F(0)] * ci.dim
                n[axis] = F(-1) if side else F(1)
                b = -(F(float(bound)) - p0[axis]) if side else F(float(bound)) - p0[axis]
            for a in range(ci.dim):
                rho[a] += lam[j] * n[a]
            v += lam[j] * b
        D = mpmath.sqrt(mpmath.fsum(max(abs(F(float(ci.world_min[a])) - p0[a]), abs(F(float(ci.world_max[a])) - p0[a])) ** 2 for a in range(ci.dim)))
        proven = v - mpmath.fsum(abs(r) for r in rho) * D
        if proven < F(PROOF_BAR):
            raise CertError("proven violation %s < 1e-6" % mpmath.nstr(proven, 12))
        if abs(proven - F(float(cert["violation"]))) > F("1e-9"):
            raise CertError("violation reported %.12g, recomputed %s" % (float(cert["violation"]), mpmath.nstr(proven, 12)))
        return float(proven)
    finally:
        mpmath.mp.dps = old
