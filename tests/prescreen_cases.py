"""Instances whose per-control-point answer is known by construction, for the prescreen (tests/prescreen_reference.py states the question).

On one free control point of a swarm instance, at a point c* inside its interval, the LSC rows are replaced by k rows whose unit normals
sum to zero (k = 2: an antiparallel pair; 3: 120 degrees apart in a plane; 4: a regular tetrahedron, 3-D only), each scaled by 0.3 .. 3
and rotated at random, with b_i = n_i.c* + s |n_i|.  Uniform weights then prove max_i (b^_i - n^_i.c) >= s at every c, and c* attains it:
t*_cp = s exactly.  'face': ONE row against a face of the interval, placed 2 s beyond it -- again t* = s.
Also: two planted control points in one instance (the lower index is the verdict's), and a row pushed s across one of the FIXED points c0,
c1, c2 -- rows the solver never reads (src/traj_optimizer.cpp:404-406), so the prescreen must stay quiet there.
"""
import numpy as np

from tests import feasibility as F
from tests import prescreen_reference as PR

SHAPES = dict(F.SHAPES, m12=(12, 3, 8))  # (M, dim, n_obs); M = 12: control points 64 .. 71 lie beyond one wavefront
S_DECIDED = (-1e-2, -1e-4, 2e-5, 1e-3, 0.4)
S_WINDOW = (2e-6, 5e-6)
COMM_RANGE = 3.0


class Case:
    """One instance (F.Instance: hdr, rows, sfc) with what was planted: kind, s, the planted control points, and t_max = max_cp t*_cp."""

    def __init__(self, inst, kind, s, cps, t_planted, t_max, expect_cp):
        self.inst, self.kind, self.s, self.cps, self.t_planted, self.t_max, self.expect_cp = inst, kind, s, cps, t_planted, t_max, expect_cp

    @property
    def label(self):
        return PR.label_of(self.t_max)


class CaseSet:
    def __init__(self, shape, M, dim, n_obs, world_min, world_max, cases, base_t):
        self.shape, self.M, self.dim, self.n_obs = shape, M, dim, n_obs
        self.world_min, self.world_max, self.cases, self.base_t = tuple(world_min), tuple(world_max), cases, base_t
        self.ci = PR.ClassInfo(M, dim, world_min, world_max, comm_range=COMM_RANGE)

    def oracle_class(self, O):
        return O.make_class(M=self.M, dim=self.dim, comm_range=COMM_RANGE, world_min=self.world_min, world_max=self.world_max)

    def desc(self, api, **kw):
        return api.make_desc(M=self.M, dim=self.dim, comm_range=COMM_RANGE, world_min=self.world_min, world_max=self.world_max, **kw)


def _unit_normals(rng, k, dim):
    """k unit normals that sum to zero, rotated at random."""
    if dim == 2:
        ph = rng.uniform(0, 2 * np.pi)
        return np.array([[np.cos(ph + 2 * np.pi * j / k), np.sin(ph + 2 * np.pi * j / k), 0.0] for j in range(k)])
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if k == 2:
        base = np.array([[1.0, 0, 0], [-1.0, 0, 0]])
    elif k == 3:
        base = np.array([[np.cos(2 * np.pi * j / 3), np.sin(2 * np.pi * j / 3), 0.0] for j in range(3)])
    else:
        base = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float) / np.sqrt(3.0)
    return base @ Q.T


def _clear(R, cp):
    for f in ("nx", "ny", "nz", "b"):
        R[f][:, cp] = 0.0


def plant(ci, h1, R, s1, cp, kind, s, rng):
    """Plants t*_cp = s on free control point cp of the instance (h1, R [n_obs, P], s1); kind: 2, 3, 4 or 'face'."""
    lo, hi = PR.interval(ci, h1, s1, cp)
    assert (hi - lo).min() >= 0.1, "the base instance's interval is too narrow to plant in"
    _clear(R, cp)
    if kind == "face":
        axis, side = int(rng.integers(ci.dim)), int(rng.integers(2))
        sc = rng.uniform(0.3, 3.0)
        n = np.zeros(3)
        n[axis] = -sc if side == 0 else sc  # against the lower face: c_k <= lo - 2 s; against the upper: c_k >= hi + 2 s
        b = -sc * (lo[axis] - 2 * s) if side == 0 else sc * (hi[axis] + 2 * s)
        R["nx"][0, cp], R["ny"][0, cp], R["nz"][0, cp], R["b"][0, cp] = n[0], n[1], n[2], b
        return
    cstar = np.zeros(3)
    cstar[:ci.dim] = 0.5 * (lo + hi) + (rng.random(ci.dim) - 0.5) * 0.2 * (hi - lo)
    if ci.dim == 2:
        cstar[2] = float(h1["p0"][2])
    U = _unit_normals(rng, kind, ci.dim)
    for j in range(kind):
        n = U[j] * rng.uniform(0.3, 3.0)
        R["nx"][j, cp], R["ny"][j, cp], R["nz"][j, cp] = n
        R["b"][j, cp] = n @ cstar + s * np.sqrt(n @ n)


def push_fixed(ci, h1, R, cp, s, rng, dt=0.2):
    """One row of neighbour 0 violated by s at the fixed control point cp in {0, 1, 2}."""
    p0, v0, a0 = (np.asarray(h1[f], float) for f in ("p0", "v0", "a0"))
    pt = [p0, p0 + v0 * dt / 5, p0 + 2 * v0 * dt / 5 + a0 * dt * dt / 20][cp]
    n = _unit_normals(rng, 2, ci.dim)[0] * rng.uniform(0.3, 3.0)
    R["nx"][0, cp], R["ny"][0, cp], R["nz"][0, cp] = n
    R["b"][0, cp] = n[:ci.dim] @ pt[:ci.dim] + s * np.sqrt(n @ n)


def rows_as_f32(rows):
    """The rows as a handle with LSCQP_ROWS_F32 reads them: rounded to float32, widened again."""
    out = rows.copy()
    for f in ("nx", "ny", "nz", "b"):
        out[f] = rows[f].astype(np.float32).astype(np.float64)
    return out


_SETS = {}


def build(api, shape, seed=11):
    """The constructed cases of one shape (cached per process)."""
    if shape in _SETS:
        return _SETS[shape]
    from lsc_dr_planner_amd import synth

    M, dim, n_obs = SHAPES[shape]
    P = M * 6
    sw = synth.Swarm(16, M=M, dim=dim, n_obs=n_obs, seed=seed)
    hdr, rows, _, sfc = api.batch_from_swarm(sw.build(), sw.n_obs, M)
    wmin, wmax = np.asarray(sw.world_min, float), np.asarray(sw.world_max, float)
    ci = PR.ClassInfo(M, dim, wmin, wmax, comm_range=COMM_RANGE)
    rng = np.random.default_rng(seed + 100)
    # a base instance whose own control points all have room (so that the planted point alone decides the label)
    for q in range(len(hdr)):
        h0, r0, s0 = F._base(hdr, rows, sfc, q, n_obs, M)
        base_t = PR.t_star_all(ci, h0, r0, s0)
        if base_t.max() <= -1e-2 - 1e-3 and min((PR.interval(ci, h0, s0, cp)[1] - PR.interval(ci, h0, s0, cp)[0]).min() for cp in range(3, P)) >= 0.1:
            break
    else:
        raise RuntimeError("no base instance with room on %s" % shape)
    cps = [3, P - 1, 64 + 3 if P > 64 else P // 2]
    kinds = [2, 3, 4, "face"] if dim == 3 else [2, 3, "face"]
    cases = []

    def fresh():
        return h0.copy(), r0.copy().reshape(n_obs, P), s0.copy()

    for rep in range(2):
        for cp in cps:
            for kind in kinds:
                for s in S_DECIDED + S_WINDOW:
                    h1, R, s1 = fresh()
                    plant(ci, h1, R, s1, cp, kind, s, rng)
                    inst = F.Instance("P", dict(kind=kind, cp=cp, s=s, rep=rep), h1, R.reshape(-1), s1)
                    t = PR.t_star_cp(ci, h1, inst.rows, s1, cp)
                    others = np.delete(base_t, cp).max()
                    cases.append(Case(inst, kind, s, [cp], t, max(t, others), cp))
    for sa, sb in ((1e-3, 0.4), (0.4, 2e-5), (2e-5, 1e-3)):  # two planted control points: the lower index is reported
        h1, R, s1 = fresh()
        ca, cb = cps[0] + 4, cps[2]
        plant(ci, h1, R, s1, ca, kinds[1], sa, rng)
        plant(ci, h1, R, s1, cb, kinds[0], sb, rng)
        inst = F.Instance("P", dict(kind="two", cp=(ca, cb), s=(sa, sb)), h1, R.reshape(-1), s1)
        ta, tb = PR.t_star_cp(ci, h1, inst.rows, s1, ca), PR.t_star_cp(ci, h1, inst.rows, s1, cb)
        cases.append(Case(inst, "two", (sa, sb), [ca, cb], ta, max(ta, tb), ca))
    for cp in range(3):  # a fixed point pushed across one row: nothing the QP reads -- the instance stays what the base is
        for s in (1e-3, 0.4):
            h1, R, s1 = fresh()
            push_fixed(ci, h1, R, cp, s, rng)
            inst = F.Instance("P", dict(kind="fixed", cp=cp, s=s), h1, R.reshape(-1), s1)
            cases.append(Case(inst, "fixed", s, [cp], PR.fixed_point_violation(ci, h1, inst.rows), base_t.max(), -1))
    _SETS[shape] = CaseSet(shape, M, dim, n_obs, wmin, wmax, cases, base_t)
    return _SETS[shape]


def to_batch(api, cases, n_obs, M):
    return F.to_batch(api, [c.inst for c in cases], n_obs, M)
