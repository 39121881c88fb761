"""Constructed position packs for neighbour selection (include/lscqp.h: lscqp_select_neighbours_device and its missions form) and the
rule itself in a few lines of numpy.

The rule: the candidates of an agent are the other agents (of its own mission, when there is a partition) whose L-infinity distance on
float32 positions is <= range (all of them when the range is <= 0); when more than n_obs are in range the n_obs nearest are kept, ties to
the smaller id, and the list is in id order, -1 padded; the count is the number in range.

Random positions have no equal distances, so every pack here is built to have them: lattices, coincident agents, agents on the faces of
a cube, and clusters far below the scale of the rest.  Each pack states what it is there for (`holds`), and that statement is checked from
the reference alone (tests/test_neighbours_cpu.py), so a pack cannot quietly stop reaching its path.  The kernel keeps up to kCap = 1024
in-range agents in LDS and ranks them there; beyond that it bisects for the threshold distance and hands the ties out window by window."""
from collections import namedtuple

import numpy as np

K_CAP = 1024  # csrc/lscgen.hip: select_neighbours_kernel, kCap

Ref = namedtuple("Ref", "nbr cnt d tie")  # lists [A][n_obs], counts [A], distances [A][N] (inf: no candidate), cut inside a tie group [A]


def reference(pos, n_obs, rng, first=0, n_agents=None, offsets=None):
    """The rule for the agents [first, first + n_agents).  offsets: a mission partition [K + 1]; ids stay global."""
    P = np.asarray(pos, dtype=np.float64).reshape(-1, 3).astype(np.float32)
    N = P.shape[0]
    A = N - first if n_agents is None else n_agents
    ids = np.arange(first, first + A)
    d = np.abs(P[ids, None, :] - P[None, :, :]).max(axis=2).astype(np.float64)  # float32 differences, widened
    out = np.arange(N)[None, :] == ids[:, None]
    if rng > 0:
        out |= d > rng
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.int64)
        mission = np.searchsorted(off, np.arange(N), side="right") - 1
        out |= mission[None, :] != mission[ids][:, None]
    d[out] = np.inf
    cnt = (~out).sum(axis=1).astype(np.int32)
    by_d = np.argsort(d, axis=1, kind="stable")  # (d, id): the ids are ascending already
    nbr = np.full((A, n_obs), -1, np.int32)
    tie = np.zeros(A, bool)
    for a in range(A):
        k = min(n_obs, int(cnt[a]))
        nbr[a, :k] = np.sort(by_d[a, :k])
        if 0 < n_obs < cnt[a]:
            tie[a] = d[a, by_d[a, n_obs - 1]] == d[a, by_d[a, n_obs]]
    return Ref(nbr, cnt, d, tie)


class Pack:
    """positions [N][3] (doubles), n_obs, range, the launched window, an optional mission partition, and what the pack is there for."""

    def __init__(self, name, pos, n_obs, rng, first=0, n_agents=None, offsets=None, holds=()):
        self.name, self.pos, self.n_obs, self.rng = name, np.ascontiguousarray(pos, dtype=np.float64), int(n_obs), float(rng)
        self.n = self.pos.shape[0]
        self.first, self.n_agents = first, self.n - first if n_agents is None else n_agents
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.int64)
        self.holds = tuple(holds)
        self._ref = {}

    def __repr__(self):
        return self.name

    def ref(self, whole=False):
        """The reference of the launched window, or of every agent (what the missions entry launches); computed once, never changed."""
        if whole not in self._ref:
            w = (0, self.n) if whole else (self.first, self.n_agents)
            r = reference(self.pos, self.n_obs, self.rng, w[0], w[1], self.offsets)
            for x in r:
                x.setflags(write=False)
            self._ref[whole] = r
        return self._ref[whole]

    def check(self):
        """Assert, from the reference alone, that the pack is what it says; returns the share of launched agents cut inside a tie group."""
        r = self.ref()
        for h in self.holds:
            h(self, r)
        return float(r.tie.mean())


# ---- what a pack can state ---------------------------------------------------------------------------------------------------------------
def rank_path(p, r):
    assert r.cnt.max() <= K_CAP, (p, r.cnt.max())


def bisection_path(p, r):
    assert r.cnt.min() > K_CAP, (p, r.cnt.min())


def ties_at_the_cut(share):
    def holds(p, r):
        assert r.tie.mean() >= share, (p, r.tie.mean())
    return holds


def counts_are(c):
    def holds(p, r):
        assert (r.cnt == c).all(), (p, r.cnt)
    return holds


def someone_at_the_range(p, r):
    assert p.rng > 0 and ((r.d == p.rng).sum(axis=1) > 0).all(), p


def list_of(agent, want):
    def holds(p, r):
        assert r.nbr[agent - p.first].tolist() == list(want), (p, r.nbr[agent - p.first])
    return holds


def no_cut(p, r):
    assert (r.cnt <= p.n_obs).all() and not r.tie.any(), p


def lattice(nx, ny, nz, h):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return g * float(h)


# ---- rank path: at most kCap in range ----------------------------------------------------------------------------------------------------
def _rank_packs():
    out = []
    L5 = lattice(5, 5, 5, 0.5)
    # in a 5 x 5 x 5 lattice the agents at L-infinity distance <= k steps are a box, so every distance is shared by a whole shell: the cut
    # falls inside a shell unless n_obs is a shell's cumulative size for that agent (7, 26, 63 at a corner; 26 in the middle ...)
    for rng in (0.0, 1.0):
        for n_obs in (1, 6, 26, 63, 64, 65, 124, 200):
            holds = [rank_path]
            if rng > 0:
                holds.append(someone_at_the_range)  # two steps of 0.5: a whole shell sits exactly at the range
            if n_obs in (1, 6):  # below the smallest first shell (7, at a corner): inside the first shell for everybody
                holds.append(ties_at_the_cut(1.0))
            if n_obs >= 124:
                holds.append(no_cut)
            out.append(Pack("lattice5-range%g-nobs%d" % (rng, n_obs), L5, n_obs, rng, holds=holds))
    same = np.tile(np.array([[0.25, -1.5, 3.0]]), (70, 1))
    out.append(Pack("coincident70", same, 8, 0.0, holds=[rank_path, ties_at_the_cut(1.0), list_of(3, [0, 1, 2, 4, 5, 6, 7, 8]),
                                                       list_of(69, range(8))]))
    out.append(Pack("coincident70-range1", same, 8, 1.0, holds=[rank_path, ties_at_the_cut(1.0), list_of(0, range(1, 9))]))
    # one agent (id 77) in the middle of a cube, 200 others on its faces: one common distance, the tie group spans four windows
    g = np.random.default_rng(11)
    F = np.float32(g.uniform(-1.5, 1.5, (201, 3))).astype(np.float64)
    F[np.arange(201), g.integers(0, 3, 201)] = g.choice([-1.5, 1.5], 201)
    F[77] = 0.0

    def one_distance(p, r):
        assert (r.d[0][np.isfinite(r.d[0])] == 1.5).all() and r.cnt[0] == 200, p
    want = [j for j in range(101) if j != 77]
    out.append(Pack("cube-faces", F, 100, 0.0, first=77, n_agents=1, holds=[rank_path, one_distance, ties_at_the_cut(1.0), list_of(77, want)]))
    out.append(Pack("cube-faces-range1.5", F, 100, 1.5, first=77, n_agents=1, holds=[rank_path, one_distance, someone_at_the_range,
                                                                                  list_of(77, want)]))
    # doubles that differ and round to one float32: in double the LARGER ids are nearer, after rounding all 20 are tied at 1
    Rd = np.zeros((21, 3))
    Rd[1:, 0] = 1.0 + (21 - np.arange(1, 21)) * 2.0 ** -40

    def tie_only_after_rounding(p, r):
        dd = np.abs(p.pos[1:, 0] - p.pos[0, 0])
        assert (np.diff(dd) < 0).all() and (r.d[0, 1:] == 1.0).all(), p
    out.append(Pack("rounding-ties", Rd, 8, 0.0, first=0, n_agents=1, holds=[rank_path, tie_only_after_rounding, list_of(0, range(1, 9))]))
    # a line of 9: total == n_obs, and total == n_obs + 1 where the two ends are tied for the middle agent (the larger id goes)
    line = lattice(9, 1, 1, 0.5)
    out.append(Pack("line9-total-is-nobs", line, 8, 0.0, holds=[rank_path, counts_are(8), no_cut]))
    out.append(Pack("line9-total-is-nobs+1", line, 7, 0.0, holds=[rank_path, counts_are(8), list_of(4, [0, 1, 2, 3, 5, 6, 7]),
                                                                list_of(0, range(1, 8))]))
    return out


# ---- the capacity edge and the bisection path ----------------------------------------------------------------------------------------------
BIG = lattice(11, 10, 10, 1.0)  # 1100 agents, every pair within 10 < 12


def cluster(delta):
    """The unit lattice with a cluster far below its scale around agent 333, which sits at (3, 3, 3): ids 0..9 at L-infinity distance delta from it, ids 1097..1099 at
    delta / 2.  With n_obs = 8 the rule keeps the three strictly nearer agents, whatever their ids, and the five smallest ids of the ten."""
    P = BIG.copy()
    c = np.array([3.0, 3.0, 3.0])  # (not a power of two: float32 is equally fine on both sides; delta / 2 = 2^-21 is still exact there)
    steps = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    P[0:10] = c + float(delta) * steps
    P[1097:1100] = c + 0.5 * float(delta) * steps[[0, 3, 6]]
    return P


def _bisection_packs():
    out = []
    w = dict(first=517, n_agents=8)  # a window of 8 that starts at no multiple of 64
    for n, path, c in ((1025, rank_path, 1024), (1026, bisection_path, 1025)):
        for rng in (0.0, 12.0):
            out.append(Pack("edge%d-range%g" % (n, rng), BIG[:n], 8, rng, holds=[path, counts_are(c), ties_at_the_cut(0.5)], **w))
    w = dict(first=455, n_agents=24)
    for rng in (0.0, 12.0):
        for n_obs in (1, 8, 64, 65, 200):
            # interior agents of the window: shells of 26, 124, 342 ... -- 1, 8, 64, 65 and 200 are inside one
            out.append(Pack("lattice1100-range%g-nobs%d" % (rng, n_obs), BIG, n_obs, rng, holds=[bisection_path, ties_at_the_cut(0.5)], **w))
        out.append(Pack("lattice1100-range%g-counts-only" % rng, BIG, 0, rng, holds=[bisection_path, counts_are(1099)], **w))
        for n_obs in (1099, 1150):
            out.append(Pack("lattice1100-range%g-nobs%d" % (rng, n_obs), BIG, n_obs, rng, holds=[bisection_path, no_cut], **w))
    w = dict(first=330, n_agents=8)
    for name, delta in (("2^-10", 2.0 ** -10), ("1e-3", np.float32(1e-3)), ("3e-4", np.float32(3e-4)), ("2^-20", 2.0 ** -20)):
        for rng in (0.0, 12.0):
            out.append(Pack("cluster-delta%s-range%g" % (name, rng), cluster(delta), 8, rng,
                            holds=[bisection_path, list_of(333, [0, 1, 2, 3, 4, 1097, 1098, 1099])], **w))
    for rng in (0.0, 12.0):  # delta = 0: thirteen agents coincide with agent 333, tied at distance 0
        out.append(Pack("cluster-delta0-range%g" % rng, cluster(0.0), 8, rng, holds=[bisection_path, list_of(333, range(8))], **w))
    # agent 70 in the middle of a cube: five agents at 0.5 (large and middle ids), everybody else on the faces at exactly 2 = the range
    g = np.random.default_rng(12)
    T = np.float32(g.uniform(-2.0, 2.0, (1100, 3))).astype(np.float64)
    T[np.arange(1100), g.integers(0, 3, 1100)] = g.choice([-2.0, 2.0], 1100)
    near = [600, 1090, 1091, 1093, 1099]
    T[near] = np.float32(g.uniform(-0.5, 0.5, (5, 3))).astype(np.float64)
    T[near, 0] = 0.5
    T[70] = 0.0

    def threshold_is_the_range(p, r):
        row = r.d[70 - p.first]
        assert np.sort(row)[p.n_obs - 1] == p.rng and (row[near] == 0.5).all() and r.cnt[70 - p.first] == 1099, p
    want = list(range(45)) + near  # 45 of the tied, then the five nearer
    out.append(Pack("threshold-at-range", T, 50, 2.0, first=70, n_agents=1, holds=[bisection_path, threshold_is_the_range, ties_at_the_cut(1.0),
                                                                                 list_of(70, want)]))
    # the hand-over of ties from window to window: agent 0 sees ids = 2 (mod 5) below 400 strictly nearer (0.5), ids = 3 (mod 11) farther (3),
    # everybody else tied at 2.  n_obs = 200 leaves 120 ties to hand out, some 46 a window: they run out inside the third window, and
    # nearer agents go on to id 397
    H = np.float32(g.uniform(-2.0, 2.0, (1100, 3))).astype(np.float64)
    idx = np.arange(1100)
    nearer = (idx % 5 == 2) & (idx < 400)
    farther = (idx % 11 == 3) & ~nearer
    H[:, 0] = np.where(nearer, 0.5, np.where(farther, 3.0, 2.0))
    H[nearer, 1:] *= 0.25
    H[0] = 0.0
    tied = [j for j in idx[1:] if not nearer[j] and not farther[j]]

    def runs_out_mid_window(p, r):
        row = r.d[0]
        assert (row[nearer] == 0.5).all() and (row[farther] == 3.0).all() and (row[tied] == 2.0).all()
        last = tied[p.n_obs - int(nearer.sum()) - 1]  # the last tied id that is kept
        assert last // 64 >= 2 and last % 64 not in (0, 63) and len(tied) > p.n_obs  # windows 0, 1 and at least one more; not at a window's end
        assert any(nearer[j] for j in range(last + 1, 400)) and any(not nearer[j] and not farther[j] for j in range((last // 64) * 64 + 64, 400))
    want = sorted(list(idx[nearer]) + tied[:200 - int(nearer.sum())])
    for rng in (0.0, 3.0):
        out.append(Pack("tie-hand-over-range%g" % rng, H, 200, rng, first=0, n_agents=1,
                        holds=[bisection_path, runs_out_mid_window, ties_at_the_cut(1.0), list_of(0, want)]))
    return out


# ---- the missions form -------------------------------------------------------------------------------------------------------------------
MISSION_OFFSETS = [0, 7, 40, 41, 1141]  # windows that start at ids that are no multiple of 64; a mission of one; 1100 agents: the bisection path


def _mission_packs():
    P = lattice(12, 10, 10, 1.0)[:1141]

    def paths(p, r):
        assert (r.cnt[:7] == 6).all() and (r.cnt[7:40] == 32).all() and r.cnt[40] == 0 and (r.cnt[41:] == 1099).all(), p
        assert r.tie[41:].mean() >= 0.5, p
    return [Pack("missions-range%g-nobs%d" % (rng, n_obs), P, n_obs, rng, offsets=MISSION_OFFSETS, holds=[paths])
            for rng in (0.0, 12.0) for n_obs in (8, 40)]


PACKS = _rank_packs() + _bisection_packs() + _mission_packs()
CLUSTER_PACKS = [p for p in PACKS if p.name.startswith("cluster-")]
