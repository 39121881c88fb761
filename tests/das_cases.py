"""Designed instances for the dual active-set phase: one QP per named thing, few rows at its optimum.  Built on the CPU, no fixture files.

Every case starts from the FREE solution of its class (the same agent with loose limits, no range rows) and then sets ONE limit to a
fraction -- 0.9, 0.8, 0.6 -- of what the free trajectory needs, so that a handful of rows bind and the case leans on the family, axis, side
and segment it is named for.  The generator asserts the oracle's status of the free and of the limited problem (a limit of 0.7 on the
communication range is infeasible on short horizons); whether the named row is active at the oracle's optimum is the premise
tests/test_das_cases.py checks through `active_rows`, which classifies rows by the STRUCTURE of the assembled row (oracle.assemble):

    one coefficient                                  interval   (corridor face, waypoint range row; lb / ub: the world box)
    two, on c[m][5] and c[0][0] of one axis          range      (the single-point range row: c[0][0] is the agent's position -- an interval
                                                                 of c[m][5] in the kernel's row list)
    two, on adjacent control points                  velocity
    three                                            acceleration
    two, on distant control points of one axis       pair
    on several axes                                  lsc

Shapes (M, dim): (5,3), (10,2), (10,3), (12,3), (2,2) with the end stop (PLANNER_LSC; the first three have fused forms), (6,3) without it
(PLANNER_DLSC), and per 3-D shape one PLANNER_RSFC instance.  Cases of one class (`Case.key`) make one batch.

Communication pairs: a swing -- v0 = -+1.5 m/s on one axis, the goal 0.6 m the other way, next_waypoint = p0, loose limits, nominal_velocity
large -- with rho = max(fraction x span, 1.02 x largest excursion from p0) holds one or two pair rows and nothing else from M = 6 up
(control points 12 and 59 at M = 10, 12 and 53 / 59 at M = 12, 12 and 35 at M = 6).  The class keeps comm_range = 3 m and the case sets the
agent's radius = comm_range / 2 - rho: the pair rows read nothing else of either.  At M = 5 the horizon is too short for these numbers; a
slower swing with a stronger pull (v0 = -+1 m/s, the goal 1.2 m the other way: the first of `SWINGS` that works) holds the pair 12 - 29
alone, on every axis and sign.  At M = 2 there is one pair and no swing isolates it: pairs are covered from M = 5 up."""
import numpy as np

SHAPES = [(5, 3, "lsc"), (10, 2, "lsc"), (10, 3, "lsc"), (12, 3, "lsc"), (2, 2, "lsc"), (6, 3, "dlsc")]
FUSED_SHAPES = [(5, 3, "lsc"), (10, 2, "lsc"), (10, 3, "lsc")]
COMM_RANGE, DT, W_C, W_T = 3.0, 0.2, 0.01, 1.0
LOOSE = dict(vmax=[30.0, 30.0, 30.0], amax=[400.0, 400.0, 400.0])
MAX_ACTIVE = 12  # rows with a multiplier at the oracle's optimum: what the launch policy's comment calls the most a feasible instance of its sweeps needed
WIDE = 30.0  # corridor faces beyond the world box: never binding unless a case moves one


class Case:
    def __init__(self, name, spec, agent, lsc=None, sfc=None, expect=None, group="main"):
        self.name, self.spec, self.agent, self.lsc, self.sfc, self.expect, self.group = name, spec, agent, lsc, sfc, expect, group

    @property
    def key(self):
        s = self.spec
        return (s["M"], s["dim"], s["planner"])

    def __repr__(self):
        return "Case(%s M%d d%d %s)" % (self.name, self.spec["M"], self.spec["dim"], self.spec["planner"])


def spec_of(M, dim, planner):
    wmin, wmax = [-20.0, -20.0, -20.0 if dim == 3 else 0.0], [20.0, 20.0, 20.0 if dim == 3 else 2.5]
    return dict(M=M, dim=dim, planner=planner, world_min=wmin, world_max=wmax, z0=0.0 if dim == 3 else 1.0)


def oracle_class(O, spec, comm_range=COMM_RANGE):
    return O.make_class(M=spec["M"], dim=spec["dim"], dt=DT, w_c=W_C, w_t=W_T, comm_range=comm_range, use_sfc=True,
                        planner_lsc={"lsc": 1, "dlsc": 0, "rsfc": 2}[spec["planner"]], world_min=spec["world_min"], world_max=spec["world_max"])


def abi_desc(A, spec, **kw):
    mode = {"lsc": A.PLANNER_LSC, "dlsc": A.PLANNER_DLSC, "rsfc": A.PLANNER_RSFC}[spec["planner"]]
    return A.make_desc(M=spec["M"], dim=spec["dim"], dt=DT, w_c=W_C, w_t=W_T, comm_range=COMM_RANGE, planner_mode=mode, use_sfc=True,
                       world_min=spec["world_min"], world_max=spec["world_max"], **kw)


def wide_box(O, spec):
    b = np.zeros(spec["M"], O.BOX_DTYPE)
    b["bmin"], b["bmax"] = [-WIDE] * 3, [WIDE] * 3
    return b


def _unit(k, s=1.0):
    e = np.zeros(3)
    e[k] = s
    return e


def _free(O, spec, **agent):
    """control points of the free solution relative to p0, (dim, M, 6)"""
    ag = O.make_agent(**dict(LOOSE, **agent))
    r = O.solve(oracle_class(O, spec, comm_range=0.0), ag, None, wide_box(O, spec))
    assert r["status"] == 0, ("free problem", spec, agent)
    x = r["x"].reshape(spec["dim"], spec["M"], 6)
    return x - np.asarray(agent["p0"], float)[:spec["dim"], None, None]


def _p0(spec):
    return np.array([0.0, 0.0, spec["z0"]])


def _hop(spec, k, s, v=0.3, dist=1.0, vn=1.0):
    """towards a goal `dist` along axis k (sign s), already moving at v along it"""
    p0 = _p0(spec)
    goal = p0 + _unit(k, s * dist) + _unit((k + 1) % spec["dim"], 0.1)
    return dict(p0=p0, v0=_unit(k, s * v), a0=np.zeros(3), goal=goal, next_waypoint=goal.copy(), nominal_velocity=vn, radius=0.15)


def _swing(spec, k, s, v=1.5, back=0.6):
    """moving away at v along axis k, the goal `back` metres the other way (sign s)"""
    p0 = _p0(spec)
    return dict(p0=p0, v0=_unit(k, -s * v), a0=np.zeros(3), goal=p0 + _unit(k, s * back), next_waypoint=p0.copy(), nominal_velocity=100.0, radius=0.15)


def _argmax_live(vals, live):
    v = np.where(live, np.abs(vals), -1.0)
    return np.unravel_index(int(np.argmax(v)), v.shape)


def dynamic_cases(O, spec):
    M, dim = spec["M"], spec["dim"]
    out = []
    for k in range(dim):
        for s in (1.0, -1.0):
            for fam, tag, v, frac in (("velocity", "", 0.3, 0.9), ("velocity", "", 0.3, 0.8), ("acceleration", "push", -0.3, 0.9),
                                      ("acceleration", "brake", 0.8, 0.9), ("acceleration", "", 0.3, 0.8)):
                a = _hop(spec, k, s, v=v)
                c = _free(O, spec, **a)[k].reshape(-1)
                if fam == "velocity":
                    d = np.array([[c[6 * m + i + 1] - c[6 * m + i] for i in range(5)] for m in range(M)]) / (DT * 0.2)
                    live = np.array([[not (m == 0 and i < 2) for i in range(5)] for m in range(M)])
                else:
                    d = np.array([[c[6 * m + i + 2] - 2 * c[6 * m + i + 1] + c[6 * m + i] for i in range(4)] for m in range(M)]) / (DT * DT * 0.05)
                    live = np.array([[not (m == 0 and i < 1) for i in range(4)] for m in range(M)])
                m, i = _argmax_live(d, live)
                lim = dict(LOOSE)
                key = "vmax" if fam == "velocity" else "amax"
                lim[key] = list(lim[key])
                lim[key][k] = frac * abs(d[m, i])
                out.append(Case("%s%s_k%d_%s_%.1f" % (fam[:3], tag and "_" + tag, k, "pos" if s > 0 else "neg", frac), spec, O.make_agent(**dict(lim, **a)),
                                expect=dict(family=fam, axis=k, side=int(d[m, i] > 0), segment=int(m))))
                out[-1].optional = frac < 0.9
    return out


def world_cases(O, spec):
    """the swing's overshoot against a face of the world box: the agent is placed so that the face sits at 0.9 of the free excursion"""
    M, dim = spec["M"], spec["dim"]
    out = []
    for k in range(dim if dim == 3 else 2):
        for s in (1.0, -1.0):
            a = _swing(spec, k, s)
            c = _free(O, spec, **a)[k]
            live = np.ones((M, 6), bool)
            live[0, :3] = False
            m, i = _argmax_live(np.where(-s * c > 0, c, 0.0), live)
            face = spec["world_max"][k] if -s > 0 else spec["world_min"][k]
            a["p0"] = a["p0"].copy()
            a["p0"][k] = face - 0.9 * c[m, i]
            shift = a["p0"] - _p0(spec)
            a["goal"], a["next_waypoint"] = a["goal"] + shift, a["next_waypoint"] + shift
            out.append(Case("world_k%d_%s" % (k, "hi" if -s > 0 else "lo"), spec, O.make_agent(**dict(LOOSE, **a)),
                            expect=dict(family="interval", axis=k, side=int(-s > 0), bound=face)))
    return out


def corridor_cases(O, spec):
    """one face of one segment's box across the way to the goal, at 0.6 of the free displacement in that segment (tests/test_gpu_parity.py:
    test_one_binding_corridor_face_per_segment_axis_and_side), early, mid-way and late in the horizon"""
    M, dim = spec["M"], spec["dim"]
    out = []
    for m in sorted({1, M // 2, M - 1}):
        for k in range(dim):
            for s in (1.0, -1.0):
                a = _hop(spec, k, s, v=0.2)
                c = _free(O, spec, **a)[k]
                reach = 0.6 * np.abs(c[m]).max()
                box = wide_box(O, spec)
                base = a["p0"][k]
                if s > 0:
                    box["bmax"][m][k] = base + reach
                else:
                    box["bmin"][m][k] = base - reach
                out.append(Case("corridor_m%d_k%d_%s" % (m, k, "hi" if s > 0 else "lo"), spec, O.make_agent(**dict(LOOSE, **a)), sfc=box,
                                expect=dict(family="interval", axis=k, side=int(s > 0), segment=m, bound=base + s * reach)))
    return out


def range_cases(O, spec):
    """the single-point range row |c[m][5] - p0| <= comm_range / 2 - radius, and the waypoint range row |c[m][5] - next_waypoint| <= comm_range / 2
    (the waypoint displaced so that its interval is the binding one), each at 0.9 of the free displacement"""
    M, dim = spec["M"], spec["dim"]
    out = []
    for k in range(dim):
        for s in (1.0, -1.0):
            a = _hop(spec, k, s)
            c5 = _free(O, spec, **a)[k][:, 5]
            m = int(np.argmax(np.abs(c5)))
            reach = 0.9 * abs(c5[m])
            b = dict(a, radius=0.5 * COMM_RANGE - reach, next_waypoint=a["p0"] + _unit(k, s * 0.9))  # (the waypoint rows: 0.9 - 1.5 .. 0.9 + 1.5)
            out.append(Case("range_k%d_%s" % (k, "hi" if s > 0 else "lo"), spec, O.make_agent(**dict(LOOSE, **b)),
                            expect=dict(family="range", axis=k, side=int(s > 0))))
            wp = a["p0"] + _unit(k, s * (reach - (0.5 * COMM_RANGE - 1e-5)))
            out.append(Case("waypoint_k%d_%s" % (k, "hi" if s > 0 else "lo"), spec, O.make_agent(**dict(LOOSE, **dict(a, next_waypoint=wp))),
                            expect=dict(family="interval", axis=k, side=int(s > 0), bound=a["p0"][k] + s * reach)))
    return out


def _pair_try(O, spec, k, s, frac, v, back):
    M = spec["M"]
    a = _swing(spec, k, s, v=v, back=back)
    c = _free(O, spec, **a)[k]
    pts = np.concatenate([c[:, 5], c[1:, 0]])
    span, exc = pts.max() - pts.min(), np.abs(c[:, 5]).max()
    rho = max(frac * span, 1.02 * exc)
    if rho >= span * (1 - 1e-3) or rho >= 0.5 * COMM_RANGE - 1e-3:  # no pair row would bind / the waypoint rows would bind first
        return None
    ag = O.make_agent(**dict(LOOSE, **dict(a, radius=0.5 * COMM_RANGE - rho)))
    r = O.solve(oracle_class(O, spec), ag, None, wide_box(O, spec))
    if r["status"] != 0:
        return None
    fams = {f["family"] for f in active_rows(O, spec, ag, None, wide_box(O, spec), r)}
    if fams != {"pair"}:
        return None
    return Case("pair_k%d_%s_%.2f" % (k, "pos" if s > 0 else "neg", frac), spec, ag, expect=dict(family="pair", axis=k, swing=(v, back)))


SWINGS = [(1.5, 0.6)] + [(v, back) for v in (1.0, 2.0, 3.0, 4.5, 6.0) for back in (0.3, 0.6, 1.2, 2.0, 3.0)]


def pair_cases(O, spec):
    M, dim = spec["M"], spec["dim"]
    out = []
    if M < 5:
        return out
    swing = next(((v, b) for (v, b) in SWINGS if _pair_try(O, spec, 0, 1.0, 0.95, v, b) is not None), None)
    assert swing is not None, ("no swing holds pair rows alone", spec)
    assert M < 10 or swing == SWINGS[0], swing
    for k in range(dim):
        for s in (1.0, -1.0):
            for frac in (0.95, 0.85):
                c = _pair_try(O, spec, k, s, frac, *swing)
                assert c is not None or frac < 0.9, ("the swing holds pair rows alone on every axis and sign", spec, k, s, frac)
                if c is not None:
                    out.append(c)
    return out


def _plane_rows(O, spec, a, planes, n_obs):
    """planes: [(slot, segment, normal, fraction of the way the free trajectory may go)] -> LSC records with p = 0 and d a float32 value
    (n'x >= d: exact in 16-byte rows)"""
    M, dim = spec["M"], spec["dim"]
    c = _free(O, spec, **a) + np.asarray(a["p0"], float)[:dim, None, None]
    L = np.zeros((n_obs, M, 6), O.LSC_DTYPE)
    for (oi, m, nrm, frac) in planes:
        n = np.asarray(nrm, float)
        vals = np.einsum("k,ki->i", n[:dim], c[:, m])
        at0 = float(n[:dim] @ np.asarray(a["p0"], float)[:dim])
        L["nrm"][oi, m] = n
        L["d"][oi, m] = float(np.float32(at0 - frac * (at0 - vals.min())))
    return L


def lsc_cases(O, spec):
    """one binding plane per obstacle slot (tests/test_gpu_parity.py: test_one_binding_lsc_plane_per_obstacle_slot): first and last slot,
    early and late segment; and a plane with an oblique normal (every component non-zero: the cross-axis path)"""
    M, dim = spec["M"], spec["dim"]
    n_obs = 4
    p0 = _p0(spec)
    goal = p0 + np.array([1.0, 0.1, 0.0])
    a = dict(p0=p0, v0=np.array([0.2, 0.0, 0.0]), a0=np.zeros(3), goal=goal, next_waypoint=goal.copy(), nominal_velocity=1.0, radius=0.15)
    obl = [-0.75, 0.5, 0.25] if dim == 3 else [-0.75, 0.5, 0.0]
    out = []
    for name, planes in (("lsc_slot0_m1", [(0, min(1, M - 1), [-1.0, 0.0, 0.0], 0.6)]), ("lsc_slot3_mlast", [(3, M - 1, [-1.0, 0.0, 0.0], 0.6)]),
                         ("lsc_slot2_mid", [(2, M // 2, [-1.0, 0.0, 0.0], 0.6)]), ("lsc_oblique_slot1_mlast", [(1, M - 1, obl, 0.6)]),
                         ("lsc_oblique_slot3_mid", [(3, M // 2, obl, 0.7)])):
        L = _plane_rows(O, spec, a, planes, n_obs)
        oi, m = planes[0][:2]
        # (by the structure of its row a plane with an axis-aligned normal IS an interval: named by its position, which no other row has)
        exp = dict(family="lsc", segment=m) if "oblique" in name else dict(family="interval", axis=0, side=1, segment=m, bound=-float(L["d"][oi, m, 0]))
        out.append(Case(name, spec, O.make_agent(n_obs=n_obs, **dict(LOOSE, **a)), lsc=L, expect=exp))
    # degenerate active sets: the same plane in two slots; a corridor face that coincides with an axis-aligned plane
    m = M - 1
    L = _plane_rows(O, spec, a, [(0, m, [-1.0, 0.0, 0.0], 0.6), (2, m, [-1.0, 0.0, 0.0], 0.6)], n_obs)
    out.append(Case("degenerate_plane_twice", spec, O.make_agent(n_obs=n_obs, **dict(LOOSE, **a)), lsc=L,
                    expect=dict(family="interval", axis=0, side=1, segment=m, bound=-float(L["d"][0, m, 0])), group="degenerate"))
    L = _plane_rows(O, spec, a, [(1, m, [-1.0, 0.0, 0.0], 0.6)], n_obs)
    box = wide_box(O, spec)
    box["bmax"][m][0] = -float(L["d"][1, m, 0])  # -x >= d  <=>  x <= -d
    out.append(Case("degenerate_face_on_plane", spec, O.make_agent(n_obs=n_obs, **dict(LOOSE, **a)), lsc=L, sfc=box, expect=None, group="degenerate"))
    return out


def terminal_cases(O, spec):
    """terminal_segments = 1, one value between, M (the phase picks its [U1|U2|G1|C] slab by it), steered by nominal_velocity, under an
    acceleration limit at 0.9 of the free peak so that steps are taken with that slab"""
    M, dim = spec["M"], spec["dim"]
    out = []
    d = float(np.sqrt(np.float32(1.0) + np.float32(0.1) ** 2))
    for ts in sorted({1, max(1, M // 2), M}):
        vn = 1e12 if ts == M else d / ((M - ts - 0.5) * DT)  # (ts = M only with no flight time to speak of: the rule rounds down)
        a = _hop(spec, 0, 1.0, vn=vn)
        cls = oracle_class(O, spec)
        assert O.terminal_segments(cls, O.make_agent(**dict(LOOSE, **a))) == ts, (spec, ts)
        c = _free(O, spec, **a)[0].reshape(-1)
        acc = np.array([[c[6 * m + i + 2] - 2 * c[6 * m + i + 1] + c[6 * m + i] for i in range(4)] for m in range(M)]) / (DT * DT * 0.05)
        live = np.array([[not (m == 0 and i < 1) for i in range(4)] for m in range(M)])
        m, i = _argmax_live(acc, live)
        lim = dict(LOOSE, amax=[0.9 * abs(acc[m, i]), 400.0, 400.0])
        out.append(Case("terminal_ts%d" % ts, spec, O.make_agent(**dict(lim, **a)),
                        expect=dict(family="acceleration", axis=0, side=int(acc[m, i] > 0), segment=int(m), ts=ts)))
    return out


def rsfc_cases(O, spec):
    """An agent under the world's ceiling that rises and falls back inside segment 0 (v0 up, a0 down): the ceiling at 0.9 of the hump's free
    height binds on c[0][3] or c[0][4] in PLANNER_LSC and must NOT bind in PLANNER_RSFC, where z of segment 0 is bounded by +-100
    (src/traj_optimizer.cpp:255-258) -- the RSFC optimum is the free one, above the ceiling."""
    if spec["dim"] != 3:
        return []
    top = spec["world_max"][2]
    a = dict(p0=np.array([0.0, 0.0, 0.0]), v0=np.array([0.0, 0.0, 0.9]), a0=np.array([0.0, 0.0, -9.5]), goal=np.array([0.5, 0.0, -0.5]),
             next_waypoint=np.array([0.5, 0.0, -0.5]), nominal_velocity=1.0, radius=0.15)
    c = _free(O, spec, **a)[2]
    hump = c[0, 3:5].max()
    assert hump > 1e-3 and c[0, 5] < 0.8 * hump and c[1:].max() < 0.8 * hump, ("the hump lies inside segment 0", c[0], c[1:].max())
    for f in ("p0", "goal", "next_waypoint"):
        a[f] = a[f] + np.array([0.0, 0.0, top - 0.9 * hump])
    i = 3 + int(np.argmax(c[0, 3:5]))
    rs = dict(spec, planner="rsfc")
    return [Case("rsfc_ceiling_binds_in_lsc", spec, O.make_agent(**dict(LOOSE, **a)), expect=dict(family="interval", axis=2, side=1, segment=0, bound=top, cp=i)),
            Case("rsfc_ceiling_relaxed", rs, O.make_agent(**dict(LOOSE, **a)), expect=dict(family=None, above=top))]


def restate(O, case, **kw):
    """tests/das_reference.py on one case (the kernel's inputs: packed rows, the header's terminal_segments)"""
    from lsc_dr_planner_amd import api as A

    from tests import das_reference as DR

    sp = case.spec
    ts = O.terminal_segments(oracle_class(O, sp), case.agent)
    lsc = None if case.lsc is None else A.pack_rows(case.lsc)
    sfc = case.sfc if case.sfc is not None else wide_box(O, sp)
    return DR.das(sp["M"], sp["dim"], DT, W_C, W_T, COMM_RANGE, sp["planner"] == "lsc", True, sp["planner"] == "rsfc", sp["world_min"], sp["world_max"],
                  case.agent, lsc, sfc, ts, **kw)


def leaving_cases(O, spec):
    """Rows that LEAVE the active set (the rotations of J): hops under several limits at once -- velocity and acceleration limits at 0.7 / 0.5 of
    the free peaks, a corridor face at 0.6 / 0.8 of the free displacement mid-way -- searched on the CPU with the restatement for instances
    that drop a row out of a list of two or more, hold at most 10 rows, carry at most 12 multipliers at the oracle's optimum and decide every step
    clearly (margin above 1e-6 m preferred).
    Up to six per shape, chosen so that a leaving row in the FIRST, a MIDDLE and the LAST position of the list is among them where one exists."""
    import itertools

    M, dim = spec["M"], spec["dim"]
    if M < 5:
        return []
    cand = []
    for v, dist, fv, fa, fc in itertools.product((0.8, -0.5), (1.0, 2.0), (0.7, 0.5, None), (0.5, None), (0.6, 0.8, None)):
        if fv is None and fa is None:
            continue
        a = _hop(spec, 0, 1.0, v=v, dist=dist)
        a["next_waypoint"] = a["p0"] + _unit(0, 0.5)
        c = _free(O, spec, **a)[0]
        cf = c.reshape(-1)
        vel = max(abs(cf[6 * m + i + 1] - cf[6 * m + i]) for m in range(M) for i in range(5) if not (m == 0 and i < 2)) / (DT * 0.2)
        acc = max(abs(cf[6 * m + i + 2] - 2 * cf[6 * m + i + 1] + cf[6 * m + i]) for m in range(M) for i in range(4) if not (m == 0 and i < 1)) / (DT * DT * 0.05)
        lim = dict(vmax=[fv * vel if fv else 30.0, 30.0, 30.0], amax=[fa * acc if fa else 400.0, 400.0, 400.0])
        box = wide_box(O, spec)
        if fc:
            box["bmax"][M // 2][0] = a["p0"][0] + fc * np.abs(c[M // 2]).max()
        case = Case("leaving_v%g_d%g_vel%s_acc%s_face%s" % (v, dist, fv, fa, fc), spec, O.make_agent(**dict(lim, **a)), sfc=box, expect=None)
        g = restate(O, case)
        pos = {("first" if l == 0 else "last" if l == kk - 1 else "middle") for (l, kk) in g["left"] if kk >= 2}
        if g["status"] == "optimal" and pos and g["peak"] <= 10:
            r = solve_oracle(O, case)
            if r["status"] == 0 and len(active_rows(O, spec, case.agent, None, box, r)) <= MAX_ACTIVE:
                cand.append((g["margin"] <= 1e-6, len(cand), pos, case))
    cand.sort(key=lambda t: t[:2])
    out, seen = [], set()
    for want in ("first", "middle", "last", None):
        for (_, _, pos, case) in cand:
            if len(out) < 6 and case not in out and (want in pos if want else True) and (want is None or want not in seen):
                out.append(case)
                seen |= pos
    return out


_CACHE = {}


def cases(O, M, dim, planner):
    """Every designed case of one shape, each with the oracle's result as `case.oracle` (the RSFC instance of a 3-D LSC shape has a class of
    its own: see Case.key).  The oracle must call every case OPTIMAL; the deeper dynamic limits (0.8) alone may turn out infeasible on a short horizon
    (M = 2), or put more than 12 rows to work on a long one (M = 12), and are then left out."""
    key = (M, dim, planner)
    if key not in _CACHE:
        spec = spec_of(M, dim, planner)
        out = dynamic_cases(O, spec) + world_cases(O, spec) + corridor_cases(O, spec) + range_cases(O, spec) + pair_cases(O, spec)
        out += lsc_cases(O, spec) + terminal_cases(O, spec) + leaving_cases(O, spec)
        if planner == "lsc":
            out += rsfc_cases(O, spec)
        kept = []
        for c in out:
            c.oracle = solve_oracle(O, c)
            if c.oracle["status"] != 0 and getattr(c, "optional", False):
                continue
            assert c.oracle["status"] == 0, (c, c.oracle["status"])
            c.rows = active_rows(O, c.spec, c.agent, c.lsc, c.sfc if c.sfc is not None else wide_box(O, c.spec), c.oracle)
            if len(c.rows) > MAX_ACTIVE and getattr(c, "optional", False):
                continue
            kept.append(c)
        assert len({c.name for c in kept if c.key == key}) == len([c for c in kept if c.key == key])
        _CACHE[key] = kept
    return _CACHE[key]


def solve_oracle(O, case):
    """the oracle on one case: its result (x polished where the fixture polishes)"""
    cls = oracle_class(O, case.spec)
    sfc = case.sfc if case.sfc is not None else wide_box(O, case.spec)
    return O.solve(cls, case.agent, case.lsc, sfc)


def active_rows(O, spec, agent, lsc, sfc, res, tol=1e-6):
    """The rows that carry a multiplier at the oracle's optimum, classified by the structure of the assembled row:
    [dict(family, axis, side, segment, cp, bound, vec)], vec = the row in the oracle's variables (G x <= h orientation)."""
    M, dim = spec["M"], spec["dim"]
    P = 6 * M
    A = O.assemble(oracle_class(O, spec), agent, lsc, sfc)
    G, h = A["G"], A["h"]
    scale = max(1.0, float(np.max(res["lam"], initial=0.0)), float(np.max(res["mu_lb"])), float(np.max(res["mu_ub"])))
    out = []

    def add(vec, rhs):
        nz = np.nonzero(vec)[0]
        ax, cp = nz // P, nz % P
        hi = int(cp.argmax())
        d = dict(axis=int(ax[0]) if len(set(ax)) == 1 else None, segment=int(cp.max() // 6), cp=int(cp.max()), vec=vec, side=int(vec[nz[hi]] > 0), bound=None)
        if len(set(ax)) > 1:
            d["family"] = "lsc"
        elif len(nz) == 1:
            d["family"], d["bound"] = "interval", rhs / vec[nz[0]]
        elif len(nz) == 3:
            d["family"] = "acceleration"
        elif cp.max() - cp.min() == 1:
            d["family"] = "velocity"
        elif cp.min() == 0:
            d["family"] = "range"
        else:
            d["family"] = "pair"
        out.append(d)

    for i in np.nonzero(res["lam"] > tol * scale)[0]:
        add(G[i], h[i])
    for v in np.nonzero(res["mu_lb"] > tol * scale)[0]:
        e = np.zeros(G.shape[1])
        e[v] = -1.0
        add(e, -A["lb"][v])
    for v in np.nonzero(res["mu_ub"] > tol * scale)[0]:
        e = np.zeros(G.shape[1])
        e[v] = 1.0
        add(e, A["ub"][v])
    return out


def matches(expect, row):
    if expect["family"] != row["family"]:
        return False
    for f in ("axis", "side", "segment", "cp"):
        if f in expect and row["family"] != "lsc" and expect[f] != row[f] and not (f in ("side", "segment") and expect["family"] == "pair"):
            return False
    if expect["family"] == "lsc":
        return expect["segment"] == row["segment"]
    if expect.get("bound") is not None and abs(row["bound"] - expect["bound"]) > 1e-9:
        return False
    return True


def signatures(spec, vecs):
    """Rows as they act on the plan's subspace (T' a per axis, normalised, rounded): rows that are the same row there -- c[m][5] and c[m+1][0]
    under one bound, a plane given twice, the end stop's three equal control points -- have one signature."""
    from tests import das_reference as DR

    M, dim = spec["M"], spec["dim"]
    P = 6 * M
    T = DR.null_space_map(M, spec["planner"] == "lsc")
    out = set()
    for v in vecs:
        red = np.concatenate([T.T @ v[k * P:(k + 1) * P] for k in range(dim)])
        out.add(tuple(np.round(red / np.linalg.norm(red), 7) + 0.0))
    return out


def restated_vectors(spec, g):
    """the restatement's active rows (a'c >= h) as vectors in the oracle's variables and orientation (G x <= h)"""
    P = 6 * spec["M"]
    out = []
    for (_, _, ent, u) in g["active"]:
        if u > 0.0:
            v = np.zeros(spec["dim"] * P)
            for (k, cp, co) in ent:
                v[k * P + cp] -= co
            out.append(v)
    return out


def rank(sigs):
    return 0 if not sigs else int(np.linalg.matrix_rank(np.array(sorted(sigs)), tol=1e-6))


def independent(sigs):
    return rank(sigs) == len(sigs)


def tight_vectors(O, case, x, tol=1e-8):
    """every row of the assembled model (and every bound) within `tol` of being active at x, as vectors in G x <= h orientation"""
    A = O.assemble(oracle_class(O, case.spec), case.agent, case.lsc, case.sfc if case.sfc is not None else wide_box(O, case.spec))
    out = [A["G"][i] for i in np.nonzero(A["h"] - A["G"] @ x <= tol)[0]]
    for v in np.nonzero(x - A["lb"] <= tol)[0]:
        e = np.zeros(len(x))
        e[v] = -1.0
        out.append(e)
    for v in np.nonzero(A["ub"] - x <= tol)[0]:
        e = np.zeros(len(x))
        e[v] = 1.0
        out.append(e)
    return out


def objective(A, x):
    """the reference's objective (x'Px + q'x + r of oracle.assemble) at x, in extended precision: in world coordinates the three terms are
    ~1e7 each for an agent 20 m from the origin and cancel to a few units"""
    xl, Pl, ql = (np.asarray(v, dtype=np.longdouble) for v in (x, A["P"], A["q"]))
    return float(xl @ (Pl @ xl) + ql @ xl + np.longdouble(A["r"]))
