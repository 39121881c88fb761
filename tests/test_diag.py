"""Failure diagnostics of the C ABI (include/lscqp.h): lscqp_dump_instance (the LP file cplex.exportModel writes in the reference,
src/traj_optimizer.cpp:45-52,103) and lscqp_diagnose (the caller's per-row debug loop, src/traj_planner.cpp:767-797, and the rows
the conflict refiner would name, src/traj_optimizer.cpp:103-137).

lscqp_diagnose evaluates eight row families -- BOUND (variable bounds = world box), SFC (corridor faces), LSC (half-spaces per obstacle
slot), VEL, ACC (dynamic limits), COMM_PAIR, COMM_WAYPOINT (communication range), EQUALITY (initial state, joins, end stop) -- and is held
to tests/diag_reference.py, a numpy restatement of the reference's model row by row, which a CPU test in turn holds to the oracle's
assembly (oracle.assemble: G, h, Aeq, beq, lb, ub).

THE TOLERANCE, once: a row has at most six terms and a right-hand side, so two fp64 evaluations of it differ by at most a small multiple
of 2^-52 * scale with scale = sum |a_j x_j| + |rhs|; every comparison here allows 8 * 2^-52 * scale (diag_reference.bound) -- for
worst[f] the largest scale in family f, because the kernel may contract multiply-adds and the restatement does not.  Counts and names are
compared exactly, under a precondition asserted on the restatement: no row within its bound of `tol`, the worst row ahead of the runner-up
by more than twice the bound (or exactly tied, where the tie rule is the subject)."""
import re

import numpy as np
import pytest

from tests import diag_cases as DC
from tests import diag_reference as DR
from tests import helpers as H

NAME_FIELDS = ("family", "obstacle", "segment", "point", "axis")
RANDOM_SEED, RANDOM_N, TOL_RANDOM = 20, 5, 1e-3
# the solver's optimum is held to 1e-8 m (tests/helpers.py: PathTol); an acceleration row scales that by 20/dt^2 = 500 over coefficients 1, 2, 1
TOL_SOLVED = 1e-8 * 500 * 4
ROW_F64 = np.dtype([("nx", "f8"), ("ny", "f8"), ("nz", "f8"), ("b", "f8")])  # packed rows widened to what the restatement reads
RSFC_TOP_WORLD = ((-6.0, -5.0, -90.0), (5.0, 6.0, 150.0))  # (a world above +100: the top z bound of segment 0 is the one in reach)
RSFC_TOP_ROWS = [(DR.BOUND, -1, 0, 4, 2, 1), (DR.BOUND, -1, 0, 3, 2, 1)]
VAR = re.compile(r"^[xyz]_\d+_\d+$")
NUM = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?$|^[+-]?inf$")


def _terms(tokens):
    """[(coef, var, var2-or-None)] and the constant of a linear / quadratic expression in CPLEX LP syntax."""
    out, const, sign, coef, i = [], 0.0, 1.0, None, 0
    while i < len(tokens):
        t = tokens[i]
        if t in "+-":
            sign = sign * (-1.0 if t == "-" else 1.0) if coef is None else (-1.0 if t == "-" else 1.0)
            if coef is not None:
                const += coef
                coef = None
        elif NUM.match(t):
            if coef is not None:
                const += coef
            coef = sign * float(t)
            sign = 1.0
        elif VAR.match(t):
            c = coef if coef is not None else sign
            coef, sign = None, 1.0
            v2 = None
            if i + 1 < len(tokens) and tokens[i + 1] == "^2":
                v2, i = t, i + 1
            elif i + 2 < len(tokens) and tokens[i + 1] == "*":
                v2, i = tokens[i + 2], i + 2
            out.append((c, t, v2))
        else:
            raise ValueError("unexpected token %r" % t)
        i += 1
    if coef is not None:
        const += coef
    return out, const


def parse_lp(path, M, dim):
    """CPLEX LP file -> dict(P, q, r, Aeq, beq, G, h, lb, ub) in the reference variable order: objective x'Px + q'x + r,
    rows `>=` negated into G x <= h (the oracle's convention)."""
    P6 = 6 * M

    def idx(v):
        a, m, i = v.split("_")
        return "xyz".index(a) * P6 + 6 * int(m) + int(i)

    nv = dim * P6
    txt = [l for l in open(path).read().split("\n") if not l.startswith("\\")]
    body = " ".join(txt)
    obj = body[body.index("Minimize") + 8:body.index("Subject To")]
    lin, quad = obj[obj.index("obj:") + 4:obj.index("[")], obj[obj.index("[") + 1:obj.index("]")]
    assert obj[obj.index("]") + 1:].split() == ["/", "2"]
    Pm, q = np.zeros((nv, nv)), np.zeros(nv)
    ltok = lin.split()
    assert ltok[-1] == "+"  # "... + [ quadratic part ] / 2"
    tl, r = _terms(ltok[:-1])
    for c, v, v2 in tl:
        assert v2 is None
        q[idx(v)] += c
    for c, v, v2 in _terms(quad.split())[0]:
        assert v2 is not None
        a, b = idx(v), idx(v2)
        Pm[a, b] += 0.25 * c if a != b else 0.5 * c  # [ ... ] / 2, and an off-diagonal product stands for both (a,b) and (b,a)
        if a != b:
            Pm[b, a] += 0.25 * c
    rows = body[body.index("Subject To") + 10:body.index("Bounds")]
    Aeq, beq, G, h = [], [], [], []
    for stmt in re.split(r"\bc\d+:", rows)[1:]:
        tok = stmt.split()
        k = [i for i, t in enumerate(tok) if t in ("=", ">=", "<=")][0]
        tl, cst = _terms(tok[:k])
        rhs = float(tok[k + 1]) - cst
        a = np.zeros(nv)
        for c, v, v2 in tl:
            a[idx(v)] += c
        if tok[k] == "=":
            Aeq.append(a), beq.append(rhs)
        elif tok[k] == "<=":
            G.append(a), h.append(rhs)
        else:
            G.append(-a), h.append(-rhs)
    lb, ub = np.full(nv, np.nan), np.full(nv, np.nan)
    for stmt in re.findall(r"(\S+ <= [xyz]_\d+_\d+ <= \S+|[xyz]_\d+_\d+ free)", body[body.index("Bounds"):]):
        tok = stmt.split()
        if tok[-1] == "free":
            lb[idx(tok[0])], ub[idx(tok[0])] = -np.inf, np.inf
        else:
            lb[idx(tok[2])], ub[idx(tok[2])] = float(tok[0]), float(tok[4])
    return dict(P=Pm, q=q, r=r, Aeq=np.array(Aeq), beq=np.array(beq), G=np.array(G), h=np.array(h), lb=lb, ub=ub)


def _swarm_case(api, oracle, M, dim, n_obs, planner_lsc=True, seed=11, planner=None, comm_range=3.0, use_sfc=True, row_format=None):
    from lsc_dr_planner_amd import synth

    sw = synth.Swarm(max(6, n_obs + 1), M=M, dim=dim, n_obs=n_obs, seed=seed)  # (an agent has at most N - 1 neighbours)
    b = sw.build()
    hdr, rows, off, sfc = api.batch_from_swarm(b, sw.n_obs, M)
    planner = planner or ("LSC" if planner_lsc else "DLSC")
    cls = oracle.make_class(M=M, dim=dim, planner_lsc={"LSC": 1, "DLSC": 0, "RSFC": 2}[planner], use_sfc=use_sfc, comm_range=comm_range,
                            world_min=sw.world_min, world_max=sw.world_max)
    sol = api.Solver(api.make_desc(M=M, dim=dim, planner_mode={"LSC": api.PLANNER_LSC, "DLSC": api.PLANNER_DLSC, "RSFC": api.PLANNER_RSFC}[planner],
                                   comm_range=comm_range, use_sfc=use_sfc, row_format=api.ROWS_F64 if row_format is None else row_format,
                                   world_min=sw.world_min, world_max=sw.world_max))
    ag, lsc, loff, sfc_o = H.swarm_oracle_inputs(oracle, sw, b)
    return sw, b, sol, cls, (hdr, rows, off, sfc), (ag, lsc, loff, sfc_o)


# lsc_mode: True / False = LSC / DLSC planner mode; a word = an LSC-mode class the dump branches on: "RSFC" (the +-100 z bounds of segment 0),
# "F32" (LSCQP_ROWS_F32: the rows are read as float32), "RANGE0" (communication_range = 0: no communication rows), "NOSFC" (use_sfc = 0, no
# boxes passed), "SHORT" (one LSC row with |n| = 3e-6, which is no row: the numbering c1..cN stays gapless)
@pytest.mark.parametrize("M,dim,n_obs,lsc_mode", [(5, 3, 3, True), (10, 2, 2, True), (4, 3, 2, False), (9, 3, 2, True), (5, 3, 3, "RSFC"),
                                                  (5, 3, 3, "F32"), (4, 3, 2, "RANGE0"), (5, 2, 2, "NOSFC"), (5, 3, 3, "SHORT")])
def test_lp_dump_is_the_reference_model_row_for_row(api, oracle, tmp_path, M, dim, n_obs, lsc_mode):
    """The LP file of an instance, parsed back, is the oracle's row-for-row assembly of populatebyrow: same objective, the same
    equality / inequality rows in the same order, the same bounds.  No device involved."""
    kw = dict(planner_lsc=lsc_mode) if isinstance(lsc_mode, bool) else {
        "RSFC": dict(planner="RSFC"), "F32": dict(row_format=api.ROWS_F32), "RANGE0": dict(comm_range=0.0), "NOSFC": dict(use_sfc=False),
        "SHORT": {}}[lsc_mode]
    sw, b, sol, cls, (hdr, rows, off, sfc), (ag, lsc, loff, sfc_o) = _swarm_case(api, oracle, M, dim, n_obs, **kw)
    q = 2
    hdr[q]["terminal_segments"] = oracle.terminal_segments(cls, ag[q:q + 1])
    rows_q = rows.reshape(len(hdr), -1)[q].copy()
    lsc_q = np.ascontiguousarray(lsc.reshape(len(hdr), -1)[q]).copy()
    if lsc_mode == "SHORT":
        e = (1 * M + 2) * 6 + 4  # obstacle 1, segment 2, point 4
        rows_q[e] = (1.8e-6, -2.4e-6, 0.0, 0.5)
        lsc_q[e]["nrm"], lsc_q[e]["p"], lsc_q[e]["d"] = (1.8e-6, -2.4e-6, 0.0), 0.0, 0.5
    if lsc_mode == "F32":  # the oracle assembles the values the handle reads: the float32 rounding of the packed rows, widened
        r32 = sol.rows_in_format(rows_q)
        assert r32.dtype == api.ROW_F32_DTYPE
        lsc_q["p"], lsc_q["d"] = 0.0, r32["b"].astype(np.float64)
        for k, f in enumerate(("nx", "ny", "nz")):
            lsc_q["nrm"][:, k] = r32[f].astype(np.float64)
    path = str(tmp_path / "QPmodel_trajOpt.lp")
    sol.dump_instance(hdr[q], rows_q, None if lsc_mode == "NOSFC" else sfc[q], path)
    got = parse_lp(path, M, dim)
    want = oracle.assemble(cls, ag[q:q + 1], lsc_q, np.ascontiguousarray(sfc_o.reshape(len(hdr), M)[q]))
    sz = want["sizes"]
    assert sz.n_lsc_skipped == (1 if lsc_mode == "SHORT" else 0) and (sz.n_comm == 0) == (lsc_mode == "RANGE0") and (sz.n_sfc == 0) == (lsc_mode == "NOSFC")
    assert got["Aeq"].shape == want["Aeq"].shape and got["G"].shape == want["G"].shape
    np.testing.assert_allclose(got["P"], want["P"], rtol=1e-13, atol=1e-9)
    np.testing.assert_allclose(got["q"], want["q"], rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(got["r"], want["r"], rtol=1e-12)
    np.testing.assert_allclose(got["Aeq"], want["Aeq"], rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(got["beq"], want["beq"], rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(got["G"], want["G"], rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(got["h"], want["h"], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(got["lb"], want["lb"])
    np.testing.assert_array_equal(got["ub"], want["ub"])
    if lsc_mode == "RSFC":
        P6 = 6 * M
        assert (got["lb"][2 * P6 + 3:2 * P6 + 6] == -100).all() and (got["ub"][2 * P6 + 3:2 * P6 + 6] == 100).all() and got["ub"][2 * P6 + 6] == sw.world_max[2]
    names = [l.split(":")[0].strip() for l in open(path) if re.match(r"^ c\d+:", l)]
    assert names == ["c%d" % (i + 1) for i in range(len(names))] and len(names) == want["sizes"].neq + want["sizes"].nineq


def test_dump_instance_argument_errors(api, tmp_path):
    sol = api.Solver(api.make_desc(M=5, dim=3))
    hdr = np.zeros(1, api.HEADER_DTYPE)
    hdr["nominal_velocity"] = 1.0
    with pytest.raises(api.LscqpError):  # the class carries SFC rows: boxes are required
        sol.dump_instance(hdr, None, None, str(tmp_path / "a.lp"))
    with pytest.raises(api.LscqpError):
        sol.dump_instance(hdr, None, np.zeros(5, api.BOX_DTYPE), str(tmp_path / "no_such_dir" / "a.lp"))
    assert api.lib().lscqp_row_family_name(api.ROW_LSC) == b"LSC" and api.lib().lscqp_row_family_name(99) == b"none"


@pytest.mark.gpu
def test_diagnose_names_the_violated_rows(api, oracle, torch_cuda):
    """lscqp_diagnose on a solved batch: nothing violated; after pushing ONE control point across an LSC plane / out of its corridor
    the report carries that row's violation in its family, and names the worst row overall (family, obstacle, segment, point, axis) as the
    restatement does.  (The dynamic limits and every other family: test_diagnose_names_each_pushed_row.)"""
    M, dim, n_obs = 5, 3, 4
    sw, b, sol, cls, (hdr, rows, off, sfc), (ag, lsc, loff, sfc_o) = _swarm_case(api, oracle, M, dim, n_obs)
    r = sol.solve_host(hdr, rows, off, sfc, x_init=api.x_init_from_swarm(b, dim))
    assert (r["status"] == 0).all()
    x = r["x"].copy()
    d = sol.diagnose_host(hdr, rows, off, sfc, x, tol=1e-8)
    assert (d["violated"] == 0).all() and (d["worst"][:, api.ROW_EQUALITY] < 1e-9).all() and (d["worst"] <= 1e-8).all()
    # every family is present and was evaluated: the smallest margins are finite
    assert np.isfinite(d["worst"]).all() and (d["worst"][:, api.ROW_LSC] > -50).all()
    P6 = 6 * M
    R = rows.reshape(len(hdr), n_obs, M, 6)
    # (1) agent 1, obstacle 2, segment 3, point 4: move the control point 0.4 m against the row's normal beyond its plane
    q, o, m, i = 1, 2, 3, 4
    row = R[q, o, m, i]
    nrm = np.array([row["nx"], row["ny"], row["nz"]])
    c = x[q].reshape(dim, P6)[:, 6 * m + i].copy()
    margin = nrm @ c - row["b"]
    c_new = c - nrm / (nrm @ nrm) * (margin + 0.4 * np.linalg.norm(nrm))
    x1 = x.copy()
    x1[q].reshape(dim, P6)[:, 6 * m + i] = c_new
    d1 = sol.diagnose_host(hdr, rows, off, sfc, x1, tol=1e-8)[q]
    lsc_viol = [(R[q, oo, m, i]["b"] - np.array([R[q, oo, m, i]["nx"], R[q, oo, m, i]["ny"], R[q, oo, m, i]["nz"]]) @ c_new, oo) for oo in range(n_obs)]
    assert d1["violated"][api.ROW_LSC] >= 1 and abs(d1["worst"][api.ROW_LSC] - max(lsc_viol)[0]) < 1e-12
    assert max(lsc_viol)[0] >= 0.4 * np.linalg.norm(nrm) - 1e-9
    # the name, unconditionally: the most violated LSC row of the restatement is that row, and the record names the restatement's worst row
    # over all families by the tie rule (c4 of segment 3 also breaks the scaled C1 / C2 joins with segment 4, by more in their units)
    cls_r = DR.make_class(M=M, dim=dim, dt=0.2, planner=DR.PLANNER_LSC, use_sfc=True, comm_range=3.0, world_min=sw.world_min, world_max=sw.world_max)
    want1, lists1, _ = DR.diagnose(cls_r, hdr, rows, off, sfc, x1, 1e-8)
    top = max((r for r in lists1[q] if r.family == DR.LSC), key=lambda r: r.value)
    assert DR.key(top) == (api.ROW_LSC, max(lsc_viol)[1], m, i, -1) and abs(top.value - max(lsc_viol)[0]) < 1e-12
    _assert_record(d1, want1[q], lists1[q], 1e-8, what="pushed across an LSC plane")
    assert tuple(d1[f] for f in NAME_FIELDS) == tuple(want1[q][f] for f in NAME_FIELDS) and d1["family"] in (api.ROW_LSC, api.ROW_EQUALITY)
    assert d1["violated"][api.ROW_EQUALITY] >= 1  # (c4 of segment 3 takes part in the C1 / C2 joins with segment 4: broken as well)
    # (2) agent 3: a point 0.25 m outside the +y face of its corridor in segment 2
    q, m, i, k = 3, 2, 3, 1
    x2 = x.copy()
    x2[q].reshape(dim, P6)[k, 6 * m + i] = sfc[q, m]["bmax"][k] + 0.25
    d2 = sol.diagnose_host(hdr, rows, off, sfc, x2, tol=1e-8)[q]
    assert d2["violated"][api.ROW_SFC] == 1 and abs(d2["worst"][api.ROW_SFC] - 0.25) < 1e-12
    # (3) the whole batch on device pointers agrees with the host-pointer entry
    import torch

    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (hdr, sol.rows_in_format(rows), off, sfc, x2)]
    dd = torch.zeros(len(hdr) * 128, dtype=torch.uint8, device=dev)
    import ctypes as C

    rc = api.lib().lscqp_diagnose_device(sol._h, len(hdr), *[C.c_void_p(v.data_ptr()) for v in t], 1e-8, C.c_void_p(dd.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    got = dd.cpu().numpy().view(api.DIAG_DTYPE)
    want = sol.diagnose_host(hdr, rows, off, sfc, x2, tol=1e-8)
    assert got.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_diagnose_an_infeasible_instance_names_the_conflict(api, oracle, torch_cuda):
    """An instance made infeasible by two opposing LSC planes on one control point: the solver reports INFEASIBLE, and the diagnosis
    of the iterate it stopped at names an LSC row of that control point (what the reference's conflict refiner prints); the oracle
    agrees on the verdict."""
    M, dim, n_obs = 5, 3, 4
    sw, b, sol, cls, (hdr, rows, off, sfc), (ag, lsc, loff, sfc_o) = _swarm_case(api, oracle, M, dim, n_obs, seed=5)
    q, m, i = 0, 2, 4
    R = rows.reshape(len(hdr), n_obs, M, 6)
    c0 = np.asarray(b["init"], dtype=np.float64)[q, m, i]
    for o, sgn in ((0, 1.0), (1, -1.0)):  # x >= cx + 0.3 and x <= cx - 0.3
        R[q, o, m, i] = (sgn, 0.0, 0.0, sgn * c0[0] + 0.3)
    L = lsc.reshape(len(hdr), n_obs, M, 6)
    for o, sgn in ((0, 1.0), (1, -1.0)):
        L[q, o, m, i]["p"], L[q, o, m, i]["nrm"], L[q, o, m, i]["d"] = (0, 0, 0), (sgn, 0, 0), sgn * c0[0] + 0.3
    r = sol.solve_host(hdr, rows, off, sfc, x_init=api.x_init_from_swarm(b, dim))
    Ro = oracle.solve_batch(cls, ag, lsc, loff, sfc_o)
    assert r["status"][q] == api.STATUS_INFEASIBLE and Ro["status"][q] != 0 and (r["status"][1:] == 0).all()
    d = sol.diagnose_host(hdr, rows, off, sfc, r["x"], tol=1e-6)[q]
    assert d["family"] == api.ROW_LSC and (d["segment"], d["point"]) == (m, i) and d["obstacle"] in (0, 1) and d["violation"] >= 0.25
    assert api.lib().lscqp_row_family_name(int(d["family"])) == b"LSC"


# ---- lscqp_diagnose against the restatement (tests/diag_reference.py), and the restatement against the oracle ------------------------------
def _oracle_names(cls, A):
    """The names of the oracle's inequality rows, walked in ITS row order: ({family: [(name, [row indices of G])]}, index of the first LSC row).
    A name's one or two rows are matched to the restatement's by position in this order alone, so a wrong order fails on the values.
    MIRRORS oracle/lscqp_oracle.c, orc_assemble, the part headed "inequalities": the SFC loop (m, face f = 2 axis + side, j), the LSC loop
    (oi, m, i; unnamed here), the dynamic limits (per k, m: the velocity pairs, then the acceleration pairs) and the communication rows
    (k, mi, m >= mi; then k, m) -- and orc_count for the sizes.  A change of the model's row order is made there, in tests/diag_reference.py:
    model, and here."""
    M, dim, sz = cls.M, cls.dim, A["sizes"]
    fixed = lambda m, i: m == 0 and i < 3
    fam = {f: {} for f in range(DR.FAMILIES)}
    g = 0
    if cls.use_sfc:
        for m in range(M):
            for f in range(2 * dim):
                for j in range(6):
                    if not fixed(m, j):
                        fam[DR.SFC].setdefault((-1, m, j, f // 2), []).append(g)
                        g += 1
    assert g == sz.n_sfc
    used = (np.abs(A["G"][g:g + sz.n_lsc]) > 0).any(axis=1)
    assert used.all()
    lsc0 = g
    g += sz.n_lsc
    for k in range(dim):
        for m in range(M):
            for i in range(5):
                if not (m == 0 and i < 2):
                    fam[DR.VEL][(-1, m, i, k)] = [g, g + 1]
                    g += 2
            for i in range(4):
                if not (m == 0 and i < 1):
                    fam[DR.ACC][(-1, m, i, k)] = [g, g + 1]
                    g += 2
    assert g == sz.n_sfc + sz.n_lsc + sz.n_vel + sz.n_acc
    if cls.comm_range > 0:
        for k in range(dim):
            for mi in range(M):
                for m in range(mi, M):
                    fam[DR.COMM_PAIR][(mi, m, 5, k)] = [g, g + 1]
                    g += 2
        for k in range(dim):
            for m in range(M):
                fam[DR.COMM_WAYPOINT][(-1, m, 5, k)] = [g, g + 1]
                g += 2
    assert g == sz.nineq
    return {f: list(v.items()) for f, v in fam.items()}, lsc0


@pytest.mark.parametrize("spec", DC.CLASSES, ids=DC.CLASS_IDS)
def test_restatement_equals_the_oracles_assembly(oracle, spec, capsys):
    """tests/diag_reference.py against oracle.assemble on random trajectories, name by name in row order: max(G x - h) over the name's one or
    two oracle rows, |Aeq x - beq|, max(lb - x, x - ub), each within 8 * 2^-52 * scale; and the row counts of every family.  Every instance
    carries one short-normal LSC row (|n| = 3e-6, b = 1e6) that neither side may count.  No device involved.
    Measured (x uniform in +-3, 5 instances per class): the largest |difference| / (2^-52 * scale) is 2.0 over the inequality families,
    0 over the bounds and 1.6 over the equalities -- the bound's 8 holds with a fourfold margin."""
    cls = DC.ref_class(spec)
    ocls = DC.oracle_class(oracle, spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, RANDOM_N, RANDOM_SEED)
    worst = {"inequalities": 0.0, "bounds": 0.0, "equalities": 0.0}
    for q in range(len(hdr)):
        L, skipped = DR.rows_of(cls, hdr[q], rows[q] if spec[5] else None, sfc[q], x[q])
        ag, lsc, box = DC.oracle_inputs(oracle, hdr[q], rows[q], sfc[q])
        A = oracle.assemble(ocls, ag, lsc, box)
        sz = A["sizes"]
        by_fam = {f: [r for r in L if r.family == f] for f in range(DR.FAMILIES)}
        assert 2 * len(by_fam[DR.SFC]) == sz.n_sfc and len(by_fam[DR.LSC]) == sz.n_lsc
        assert 2 * (len(by_fam[DR.VEL]) + len(by_fam[DR.ACC])) == sz.n_vel + sz.n_acc
        assert 2 * (len(by_fam[DR.COMM_PAIR]) + len(by_fam[DR.COMM_WAYPOINT])) == sz.n_comm
        assert len(by_fam[DR.EQUALITY]) == sz.neq and skipped == sz.n_lsc_skipped == (1 if spec[5] else 0)
        gx = A["G"] @ x[q] - A["h"] if sz.nineq else np.zeros(0)
        names, lsc0 = _oracle_names(cls, A)
        for f in (DR.SFC, DR.VEL, DR.ACC, DR.COMM_PAIR, DR.COMM_WAYPOINT):
            assert [DR.key(r)[1:] for r in by_fam[f]] == [nm for nm, _ in names[f]], "family %d is not in populatebyrow order" % f
            for r, (_, idx) in zip(by_fam[f], names[f]):
                err = abs(r.value - gx[idx].max())
                worst["inequalities"] = max(worst["inequalities"], err / (DR.U * r.scale))
                assert err <= DR.bound(r.scale), (r, gx[idx])
        for j, r in enumerate(by_fam[DR.LSC]):  # (the oracle's LSC rows carry no name: by position)
            err = abs(r.value - gx[lsc0 + j])
            worst["inequalities"] = max(worst["inequalities"], err / (DR.U * r.scale))
            assert err <= DR.bound(r.scale), (r, gx[lsc0 + j])
        eq = np.abs(A["Aeq"] @ x[q] - A["beq"])
        for j, r in enumerate(by_fam[DR.EQUALITY]):
            err = abs(r.value - eq[j])
            worst["equalities"] = max(worst["equalities"], err / (DR.U * r.scale))
            assert err <= DR.bound(r.scale), (r, eq[j])
        bounded = np.flatnonzero(np.isfinite(A["lb"]))
        assert len(bounded) == len(by_fam[DR.BOUND]) and np.isfinite(A["ub"][bounded]).all()
        for r, v in zip(by_fam[DR.BOUND], bounded):
            assert v == r.axis * 6 * cls.M + 6 * r.segment + r.point
            err = abs(r.value - max(A["lb"][v] - x[q][v], x[q][v] - A["ub"][v]))
            worst["bounds"] = max(worst["bounds"], err / (DR.U * r.scale))
            assert err <= DR.bound(r.scale), r
        assert DR.record(L, TOL_RANDOM)["worst"][DR.LSC] < 1e3  # (the short-normal row, violated by 1e6, is no row)
    with capsys.disabled():
        print("\n[diag] restatement vs oracle, |difference| / (2^-52 scale), %s: %s" % (DC.CLASS_IDS[DC.CLASSES.index(spec)], worst))


def test_restatement_record_rules():
    """The record the restatement derives from a list of rows: the tie rule, the non-finite rule, a family without rows."""
    rows = [DR.Row(DR.LSC, 1, 0, 3, -1, 0.5, 1.0), DR.Row(DR.BOUND, -1, 2, 1, 0, 0.5, 1.0), DR.Row(DR.BOUND, -1, 1, 4, 2, 0.5, 1.0),
            DR.Row(DR.VEL, -1, 0, 2, 0, -0.1, 1.0)]
    d = DR.record(rows, 0.5)
    assert tuple(d[f] for f in NAME_FIELDS) == (DR.BOUND, -1, 1, 4, 2) and d["violation"] == 0.5 and d["violated"].sum() == 0
    assert DR.record(rows, np.nextafter(0.5, 0))["violated"].tolist() == [2, 0, 1, 0, 0, 0, 0, 0] and DR.runner_up(rows) == -0.1
    assert d["worst"][DR.SFC] == 0 and d["worst"][DR.VEL] == -0.1
    d = DR.record(rows + [DR.Row(DR.EQUALITY, -1, 1, 0, 0, float("nan"), 1.0), DR.Row(DR.ACC, -1, 1, 0, 0, float("inf"), 1.0)], 1e-3)
    assert tuple(d[f] for f in NAME_FIELDS) == (DR.ACC, -1, 1, 0, 0) and d["violation"] == np.inf
    assert d["worst"][DR.EQUALITY] == np.inf and d["violated"][DR.EQUALITY] == 1 and d["violated"][DR.ACC] == 1
    assert DR.record([], 0.0)["family"] == -1 and DR.DIAG_DTYPE == DC.api().DIAG_DTYPE


def _restated(cls, sol, hdr, rows, off, sfc, x, tol):
    """The restatement on the values the handle reads (float32 rows widened for an LSCQP_ROWS_F32 handle)."""
    wide = None
    if rows is not None:
        r = sol.rows_in_format(rows)
        wide = np.zeros(r.shape, ROW_F64)
        for f in ("nx", "ny", "nz", "b"):
            wide[f] = r[f].astype(np.float64)
    return DR.diagnose(cls, hdr, wide, off, sfc, x, tol)


def _assert_record(got, want, L, tol, names=True, what=""):
    """One kernel record against the restatement's: counts exactly, worst[f] within the bound of the family's largest scale, and -- under the
    precondition that the worst row leads by more than twice the bound, or ties exactly -- the name and its violation.  Returns the largest
    |worst difference| / (2^-52 * scale) seen."""
    ratio = 0.0
    for r in L:  # precondition of the counts: no row within its own bound of tol
        assert not np.isfinite(r.value) or not abs(DR.effective(r.value) - tol) <= DR.bound(r.scale), (what, "a row sits at tol", r)
    assert got["violated"].tolist() == want["violated"].tolist(), (what, got, want)
    for f in range(DR.FAMILIES):
        s = DR.family_scale(L, f)
        if np.isinf(want["worst"][f]) or s == 0.0:
            assert got["worst"][f] == want["worst"][f], (what, f, got, want)
        else:
            ratio = max(ratio, abs(got["worst"][f] - want["worst"][f]) / (DR.U * s))
            assert abs(got["worst"][f] - want["worst"][f]) <= DR.bound(s), (what, f, got["worst"][f], want["worst"][f])
    assert got["reserved"] == 0
    if names:
        best = DR.argmax_set(L)
        if best and np.isfinite(DR.effective(best[0].value)):
            smax = max(r.scale for r in L)
            tied = len(best) > 1
            assert all(r.value == best[0].value for r in best)
            assert DR.effective(best[0].value) - DR.runner_up(L) > 2 * DR.bound(smax), (what, "the worst row does not lead", best[0], DR.runner_up(L))
            assert abs(got["violation"] - want["violation"]) <= (0.0 if tied else DR.bound(best[0].scale)), (what, got, want)
        else:
            assert got["violation"] == want["violation"], (what, got, want)
        assert tuple(got[f] for f in NAME_FIELDS) == tuple(want[f] for f in NAME_FIELDS), (what, got, want)
    return ratio


@pytest.mark.parametrize("spec", DC.CLASSES, ids=DC.CLASS_IDS)
def test_random_trajectories_preconditions_hold_on_the_cpu(spec):
    """The seeds of the random GPU case: on the restatement no row sits within its bound of tol, every family with rows is violated, and the
    worst row leads.  (CPU: a seed is chosen here, not on the device.)"""
    cls = DC.ref_class(spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, RANDOM_N, RANDOM_SEED)
    want, lists, _ = DR.diagnose(cls, hdr, rows.reshape(-1), off, sfc, x, TOL_RANDOM)
    for q, L in enumerate(lists):
        _assert_record(want[q], want[q], L, TOL_RANDOM)
        present = sorted(set(r.family for r in L))
        assert present == [f for f in range(DR.FAMILIES) if (f != DR.SFC or spec[3]) and (f != DR.LSC or spec[5]) and (f not in (5, 6) or spec[4] > 0)]
        assert all(want[q]["violated"][f] > 0 for f in present)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", DC.CLASSES, ids=DC.CLASS_IDS)
def test_diagnose_random_trajectories_against_the_restatement(api, torch_cuda, spec, capsys):
    """x uniform in +-3, tol = 1e-3: every family is violated; worst[f], violated[f] and the named row against the restatement.
    Measured on the MI355X: the largest |worst[f] difference| / (2^-52 * scale) is 1.14 over the five classes (NOTES.md, section 34)."""
    cls, sol = DC.ref_class(spec), DC.solver(spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, RANDOM_N, RANDOM_SEED)
    has_rows = spec[5] > 0
    got = sol.diagnose_host(hdr, rows.reshape(-1) if has_rows else None, off if has_rows else None, sfc if spec[3] else None, x, tol=TOL_RANDOM)
    want, lists, _ = _restated(cls, sol, hdr, rows.reshape(-1) if has_rows else None, off, sfc, x, TOL_RANDOM)
    ratio = max(_assert_record(got[q], want[q], lists[q], TOL_RANDOM, what="instance %d" % q) for q in range(len(hdr)))
    with capsys.disabled():
        print("\n[diag] kernel vs restatement, largest |worst difference| / (2^-52 scale), %s: %.3f" % (DC.CLASS_IDS[DC.CLASSES.index(spec)], ratio))
    # the same call ten times: identical bytes
    for _ in range(9):
        again = sol.diagnose_host(hdr, rows.reshape(-1) if has_rows else None, off if has_rows else None, sfc if spec[3] else None, x, tol=TOL_RANDOM)
        assert again.tobytes() == got.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("spec", DC.CLASSES, ids=DC.CLASS_IDS)
def test_diagnose_a_solved_batch_against_the_restatement(api, oracle, torch_cuda, spec):
    """The optimum of solve_host on a small swarm, in each of the five classes: no row is counted, and worst[f] is the restatement's smallest
    margin negated, family by family -- which a kernel that skipped rows would not give.  A class without corridors passes sfc = NULL, one
    without obstacles rows = NULL; a family the class does not have reports 0."""
    M, dim, planner, use_sfc, rng, n_obs = spec
    sw, b, sol, ocls, (hdr, rows, off, sfc), _ = _swarm_case(api, oracle, M, dim, n_obs, planner=planner, comm_range=rng, use_sfc=use_sfc)
    assert sw.n_obs == n_obs and (hdr["n_obs"] == n_obs).all()
    rows, off, sfc = (rows if n_obs else None), (off if n_obs else None), (sfc if use_sfc else None)
    r = sol.solve_host(hdr, rows, off, sfc, x_init=api.x_init_from_swarm(b, dim))
    assert (r["status"] == 0).all()
    cls = DR.make_class(M=M, dim=dim, dt=0.2, planner=sol.desc.planner_mode, use_sfc=use_sfc, comm_range=rng, world_min=sw.world_min,
                        world_max=sw.world_max)
    got = sol.diagnose_host(hdr, rows, off, sfc, r["x"], tol=TOL_SOLVED)
    want, lists, _ = _restated(cls, sol, hdr, rows, off, sfc, r["x"], TOL_SOLVED)
    assert (got["violated"] == 0).all() and (want["violated"] == 0).all()
    present = [f for f in range(DR.FAMILIES) if (f != DR.SFC or use_sfc) and (f != DR.LSC or n_obs) and (f not in (DR.COMM_PAIR, DR.COMM_WAYPOINT) or rng > 0)]
    for q in range(len(hdr)):
        _assert_record(got[q], want[q], lists[q], TOL_SOLVED, names=False, what="instance %d" % q)
        assert np.isfinite(want[q]["worst"]).all() and sorted(set(r.family for r in lists[q])) == present
        assert all(got[q]["worst"][f] == 0 for f in range(DR.FAMILIES) if f not in present)


def _pushed(spec, names, world=None):
    cls, hdr, rows, off, sfc, x = DC.pushed_batch(spec, names, world=world)
    has_rows = spec[5] > 0
    return cls, hdr, (rows.reshape(-1) if has_rows else None), (off if has_rows else None), (sfc if spec[3] else None), x


def _check_pushed(cls, names, want, lists):
    """Preconditions of a pushed batch, on the restatement: instance q's worst row is names[q], by 0.3 in its units, alone and in the lead."""
    for q, name in enumerate(names):
        best = DR.argmax_set(lists[q])
        assert len(best) == 1 and DR.key(best[0]) == tuple(name[:5]), (name, best[:3])
        assert abs(best[0].value - 0.3) < 1e-9 and DR.runner_up(lists[q]) < 0.29, (name, best[0], DR.runner_up(lists[q]))
        assert want[q]["violated"][name[0]] >= 1  # (its neighbours may be violated too, by less)


@pytest.mark.parametrize("spec", DC.CLASSES, ids=DC.CLASS_IDS)
def test_pushed_rows_are_the_unique_worst_on_the_cpu(spec):
    names = DC.chosen_rows(spec)
    assert len(names) <= 67 and len(set(names)) == len(names)
    cls, hdr, rows, off, sfc, x = _pushed(spec, names)
    want, lists, _ = DR.diagnose(cls, hdr, rows, off, sfc, x, 1e-6)
    _check_pushed(cls, names, want, lists)
    fams = set(n[0] for n in names)
    assert fams == set(r.family for r in lists[0])  # every family the class has is pushed


@pytest.mark.gpu
@pytest.mark.parametrize("spec", DC.CLASSES, ids=DC.CLASS_IDS)
def test_diagnose_names_each_pushed_row(api, torch_cuda, spec):
    """One instance per chosen row (tests/diag_cases.py: chosen_rows -- every family in a first, a middle and the last segment, on axis 0 and
    the last axis, both faces / signs, the last obstacle slot, the RSFC z bound of segment 0, every kind of equality): the row is the unique
    worst by 0.3 in its units; all five name fields and the violation against the restatement."""
    names = DC.chosen_rows(spec)
    cls, hdr, rows, off, sfc, x = _pushed(spec, names)
    sol = DC.solver(spec, DC.wide_world(spec))
    want, lists, _ = _restated(cls, sol, hdr, rows, off, sfc, x, 1e-6)
    _check_pushed(cls, names, want, lists)
    got = sol.diagnose_host(hdr, rows, off, sfc, x, tol=1e-6)
    for q, name in enumerate(names):
        _assert_record(got[q], want[q], lists[q], 1e-6, what=str(name))
        assert tuple(got[q][f] for f in NAME_FIELDS) == tuple(name[:5])


def test_rsfc_top_rows_are_the_unique_worst_on_the_cpu():
    cls, hdr, rows, off, sfc, x = _pushed(DC.CLASSES[3], RSFC_TOP_ROWS, RSFC_TOP_WORLD)
    want, lists, _ = DR.diagnose(cls, hdr, rows, off, sfc, x, 1e-6)
    _check_pushed(cls, RSFC_TOP_ROWS, want, lists)


@pytest.mark.gpu
def test_diagnose_names_the_rsfc_top_bound_of_segment_0(api, torch_cuda):
    """RSFC: z <= +100 on segment 0 whatever the world says (here its top is at 150); chosen_rows pushes the -100 side."""
    spec = DC.CLASSES[3]
    cls, hdr, rows, off, sfc, x = _pushed(spec, RSFC_TOP_ROWS, RSFC_TOP_WORLD)
    sol = DC.solver(spec, RSFC_TOP_WORLD)
    want, lists, _ = _restated(cls, sol, hdr, rows, off, sfc, x, 1e-6)
    _check_pushed(cls, RSFC_TOP_ROWS, want, lists)
    got = sol.diagnose_host(hdr, rows, off, sfc, x, tol=1e-6)
    for q, name in enumerate(RSFC_TOP_ROWS):
        _assert_record(got[q], want[q], lists[q], 1e-6, what=str(name))
        assert tuple(got[q][f] for f in NAME_FIELDS) == tuple(name[:5]) and abs(got[q]["violation"] - 0.3) < 1e-9


@pytest.mark.gpu
def test_diagnose_batch_mapping(api, torch_cuda):
    """n = 67 instances, each with a different pushed row: record q is instance q's; and n = 1 gives that instance's record."""
    spec = DC.CLASSES[0]
    names = DC.chosen_rows(spec)
    names = (names + [b for b in DC.interior_bound_rows(spec) if b[:5] not in set(n[:5] for n in names)])[:67]
    assert len(names) == 67 and len(set(n[:5] for n in names)) == 67
    cls, hdr, rows, off, sfc, x = _pushed(spec, names)
    sol = DC.solver(spec, DC.wide_world(spec))
    want, lists, _ = _restated(cls, sol, hdr, rows, off, sfc, x, 1e-6)
    _check_pushed(cls, names, want, lists)
    got = sol.diagnose_host(hdr, rows, off, sfc, x, tol=1e-6)
    for q, name in enumerate(names):
        assert tuple(got[q][f] for f in NAME_FIELDS) == tuple(name[:5]), (q, name, got[q])
    P = 6 * spec[0] * spec[5]
    for q in (0, 41, 66):
        one = sol.diagnose_host(hdr[q:q + 1], rows[q * P:(q + 1) * P], np.array([0, P], np.uint64), sfc[q:q + 1], x[q:q + 1], tol=1e-6)
        assert one.tobytes() == got[q:q + 1].tobytes()


# ---- edges: each compares the whole record with the restatement ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_diagnose_ragged_obstacle_counts_and_poison_rows(api, torch_cuda):
    """Obstacle counts (0, 1, 4, 11) read through row_offsets that are no common multiple; the rows between an instance's n_obs and the next
    offset are violated by 1e6 and must not appear."""
    spec = DC.CLASSES[0]
    M, P = spec[0], 6 * spec[0]
    counts, gaps = [0, 1, 4, 11], [7, 5, 13, 3]
    cls, sol = DC.ref_class(spec), DC.solver(spec)
    hdr, rows11, _, sfc, x = DC.random_batch((spec[0], spec[1], spec[2], spec[3], spec[4], 11), 4, 5, short_normal=False)
    hdr["n_obs"] = counts
    off = DC.offsets(counts, M, gaps)
    flat = np.zeros(int(off[-1]), api.ROW_DTYPE)
    flat[:] = (1.0, 0.0, 0.0, 1e6)  # poison
    for q, c in enumerate(counts):
        flat[int(off[q]):int(off[q]) + c * P] = rows11[q].reshape(-1)[:c * P]
    got = sol.diagnose_host(hdr, flat, off, sfc, x, tol=TOL_RANDOM)
    want, lists, _ = _restated(cls, sol, hdr, flat, off, sfc, x, TOL_RANDOM)
    for q in range(4):
        _assert_record(got[q], want[q], lists[q], TOL_RANDOM, what="instance %d" % q)
    assert (got["worst"][:, DR.LSC] < 1e3).all() and got["worst"][0, DR.LSC] == 0 and got["violated"][0, DR.LSC] == 0


@pytest.mark.gpu
def test_diagnose_no_obstacles_null_rows(api, torch_cuda):
    """n_obs = 0 with rows = NULL and row_offsets = NULL through the host entry."""
    spec = DC.CLASSES[4]
    cls, sol = DC.ref_class(spec), DC.solver(spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, 3, 8)
    got = sol.diagnose_host(hdr, None, None, sfc, x, tol=TOL_RANDOM)
    want, lists, _ = _restated(cls, sol, hdr, None, None, sfc, x, TOL_RANDOM)
    for q in range(3):
        _assert_record(got[q], want[q], lists[q], TOL_RANDOM, what="instance %d" % q)
    assert (got["worst"][:, DR.LSC] == 0).all() and (got["violated"][:, DR.LSC] == 0).all() and (got["family"] != DR.LSC).all()


@pytest.mark.gpu
def test_diagnose_short_normals(api, torch_cuda):
    """A row with |n| = 3e-6 violated by 1e6 does not exist (:409-411); the same row with |n| = 2e-5 is named."""
    spec = DC.CLASSES[0]
    cls, sol = DC.ref_class(spec), DC.solver(spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, 2, 9, short_normal=False)
    o, m, i = 3, 2, 5
    for length, named in ((3e-6, False), (2e-5, True)):
        rows[1, o, m, i] = (0.6 * length, 0.0, -0.8 * length, 1e6)
        got = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=TOL_RANDOM)
        want, lists, skipped = _restated(cls, sol, hdr, rows.reshape(-1), off, sfc, x, TOL_RANDOM)
        assert skipped == [0, 0 if named else 1]
        for q in range(2):
            _assert_record(got[q], want[q], lists[q], TOL_RANDOM, what="|n| = %g, instance %d" % (length, q))
        if named:
            assert tuple(got[1][f] for f in NAME_FIELDS) == (DR.LSC, o, m, i, -1) and abs(got[1]["violation"] - 1e6) < 1.0
        else:
            assert got[1]["worst"][DR.LSC] < 1e3 and got[1]["violation"] < 1e5


@pytest.mark.gpu
def test_diagnose_f32_rows(api, torch_cuda):
    """LSCQP_ROWS_F32: the record equals, byte for byte, that of an fp64 handle on the widened values, and the restatement on those values."""
    spec = DC.CLASSES[0]
    cls, sol32, sol64 = DC.ref_class(spec), DC.solver(spec, row_format=api.ROWS_F32), DC.solver(spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, 4, 10)
    r32 = sol32.rows_in_format(rows.reshape(-1))
    assert r32.dtype == api.ROW_F32_DTYPE
    wide = np.zeros(r32.shape, api.ROW_DTYPE)
    for f in ("nx", "ny", "nz", "b"):
        wide[f] = r32[f].astype(np.float64)
    assert (wide["b"] != rows.reshape(-1)["b"]).any()
    got32 = sol32.diagnose_host(hdr, r32, off, sfc, x, tol=TOL_RANDOM)
    got64 = sol64.diagnose_host(hdr, wide, off, sfc, x, tol=TOL_RANDOM)
    assert got32.tobytes() == got64.tobytes()
    want, lists, _ = DR.diagnose(cls, hdr, wide, off, sfc, x, TOL_RANDOM)
    for q in range(4):
        _assert_record(got32[q], want[q], lists[q], TOL_RANDOM, what="instance %d" % q)


@pytest.mark.gpu
def test_diagnose_planar_class_ignores_nz(api, torch_cuda):
    """dim = 2: a row with a large nz gives the value of the planar row."""
    spec = DC.CLASSES[1]
    cls, sol = DC.ref_class(spec), DC.solver(spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, 3, 12, short_normal=False)
    rows["nz"] = 0.0
    flat0 = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=TOL_RANDOM)
    rows["nz"] = np.random.default_rng(1).uniform(500, 1000, rows.shape)
    got = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=TOL_RANDOM)
    assert got.tobytes() == flat0.tobytes()
    want, lists, _ = _restated(cls, sol, hdr, rows.reshape(-1), off, sfc, x, TOL_RANDOM)
    for q in range(3):
        _assert_record(got[q], want[q], lists[q], TOL_RANDOM, what="instance %d" % q)


@pytest.mark.gpu
def test_diagnose_classes_without_communication_or_corridor_rows(api, torch_cuda):
    """communication_range = 0: families 5 and 6 have worst = 0, violated = 0 and are never named, though every pair is 6 m apart;
    use_sfc = 0: family 1 likewise, with d_sfc = NULL accepted."""
    for spec, absent in ((DC.CLASSES[2], (DR.COMM_PAIR, DR.COMM_WAYPOINT)), (DC.CLASSES[3], (DR.SFC,))):
        cls, sol = DC.ref_class(spec), DC.solver(spec)
        hdr, rows, off, sfc, x = DC.random_batch(spec, 3, 13)
        if spec[4] == 0:
            hdr["vmax"], hdr["amax"] = 1e6, 1e6
            x.reshape(3, spec[1], spec[0], 6)[:, :, :, 5] = 3.0  # (the pair and waypoint rows would be the worst)
            x.reshape(3, spec[1], spec[0], 6)[:, :, :, 0] = -3.0
        got = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc if spec[3] else None, x, tol=TOL_RANDOM)
        want, lists, _ = _restated(cls, sol, hdr, rows.reshape(-1), off, sfc, x, TOL_RANDOM)
        for q in range(3):
            _assert_record(got[q], want[q], lists[q], TOL_RANDOM, what="instance %d" % q)
            for f in absent:
                assert got[q]["worst"][f] == 0 and got[q]["violated"][f] == 0 and got[q]["family"] != f


def _tail_shift(spec, world, seg, axis, by, hover=DC.HOVER):
    """A hover instance whose control points from (seg, 3) on are translated by `by` along `axis`: every equality holds exactly (the joins are
    differences), and all numbers are exactly representable."""
    M, dim = spec[0], spec[1]
    g = np.random.default_rng(4)
    hdr, rows, sfc, x = DC.hover_instance(spec, np.asarray(hover, dtype=np.float64), g)
    X = x.reshape(dim, 6 * M)
    X[axis, 6 * seg + 3:] += by
    return hdr, rows, sfc, x


@pytest.mark.gpu
def test_diagnose_strictness_of_tol(api, torch_cuda):
    """A control point at world_max + 0.25, exactly: with tol = 0.25 the row is not counted, with tol = nextafter(0.25, 0) it is."""
    spec, world = DC.CLASSES[2], DC.WORLD_WIDE
    M = spec[0]
    sol = DC.solver(spec, world)
    hdr, rows, sfc, x = _tail_shift(spec, world, M - 1, 0, 0.0)
    x.reshape(spec[1], 6 * M)[0, 6 * (M - 1) + 4] = world[1][0] + 0.25
    hdr, sfc, x = hdr.reshape(1), sfc.reshape(1, M), x.reshape(1, -1)
    off = DC.offsets([spec[5]], M)
    at = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=0.25)[0]
    below = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=np.nextafter(0.25, 0))[0]
    assert at["worst"][DR.BOUND] == 0.25 and at["violated"][DR.BOUND] == 0 and below["violated"][DR.BOUND] == 1
    assert tuple(at[f] for f in NAME_FIELDS) == (DR.BOUND, -1, M - 1, 4, 0) and at["violation"] == 0.25
    want, lists, _ = _restated(DC.ref_class(spec, world), sol, hdr, rows.reshape(-1), off, sfc, x, 0.25)
    assert want[0]["violated"][DR.BOUND] == 0 and want[0]["worst"][DR.BOUND] == 0.25


@pytest.mark.gpu
def test_diagnose_tie_rule(api, torch_cuda):
    """Among rows of equal violation the named row is the least in (family, obstacle, segment, point, axis) (include/lscqp.h).
    (a) a corridor face on the world face, a point 0.25 beyond both: BOUND, not SFC;
    (b) control points of several segments equally far outside: the lowest segment -- (0, 3) on axis 1 of a 10-segment class sits in lane 63,
        the points of segment 1 in lanes 2..7;
    (c) an LSC row (lane 3) and a BOUND row of another control point (lane 21), both at exactly 0.5: BOUND."""
    # (a), (c): class 2 (M = 4, DLSC, no communication rows); the tail from (M - 1, 3) is free of joins and end stops
    spec, world = DC.CLASSES[2], DC.WORLD_WIDE
    M, dim = spec[0], spec[1]
    cls, sol = DC.ref_class(spec, world), DC.solver(spec, world)
    off = DC.offsets([spec[5]], M)
    margin = world[1][0] - DC.HOVER[0]
    hdr, rows, sfc, x = _tail_shift(spec, world, M - 1, 0, margin + 0.25)
    sfc["bmax"][:, 0] = world[1][0]
    args = (hdr.reshape(1), rows.reshape(-1), off, sfc.reshape(1, M), x.reshape(1, -1))
    got = sol.diagnose_host(*args, tol=1e-6)[0]
    want, lists, _ = _restated(cls, sol, *args, 1e-6)
    assert len(DR.argmax_set(lists[0])) == 6 and set(r.family for r in DR.argmax_set(lists[0])) == {DR.BOUND, DR.SFC}
    _assert_record(got, want[0], lists[0], 1e-6, what="(a)")
    assert tuple(got[f] for f in NAME_FIELDS) == (DR.BOUND, -1, M - 1, 3, 0) and got["violation"] == 0.25
    hdr, rows, sfc, x = _tail_shift(spec, world, M - 1, 0, margin + 0.5)
    rows[0, 0, 3] = (0.0, 0.0, 1.0, DC.HOVER[2] + 0.5)  # z >= hover + 0.5 on control point (0, 3), which hovers: violated by exactly 0.5
    args = (hdr.reshape(1), rows.reshape(-1), off, sfc.reshape(1, M), x.reshape(1, -1))
    got = sol.diagnose_host(*args, tol=1e-6)[0]
    want, lists, _ = _restated(cls, sol, *args, 1e-6)
    assert [DR.key(r) for r in DR.argmax_set(lists[0])] == [(DR.BOUND, -1, M - 1, i, 0) for i in (3, 4, 5)] + [(DR.LSC, 0, 0, 3, -1)]
    _assert_record(got, want[0], lists[0], 1e-6, what="(c)")
    assert tuple(got[f] for f in NAME_FIELDS) == (DR.BOUND, -1, M - 1, 3, 0) and got["violation"] == 0.5
    assert got["worst"][DR.LSC] == 0.5 and got["violated"][DR.LSC] == 1 and got["violated"][DR.BOUND] == 3
    # (b): class 3 (M = 10, dim = 3, no corridor rows); the whole trajectory from (0, 3) on is 0.25 beyond the world's +y face
    spec = DC.CLASSES[3]
    world = DC.wide_world(spec)
    M = spec[0]
    cls, sol = DC.ref_class(spec, world), DC.solver(spec, world)
    hover = (DC.HOVER[0], world[1][1] - 0.25, DC.HOVER[2])  # (close to the face: the shift stays inside the communication range)
    hdr, rows, sfc, x = _tail_shift(spec, world, 0, 1, 0.5, hover)
    args = (hdr.reshape(1), rows.reshape(-1), DC.offsets([spec[5]], M), None, x.reshape(1, -1))
    got = sol.diagnose_host(*args, tol=1e-6)[0]
    want, lists, _ = _restated(cls, sol, *args, 1e-6)
    assert len(DR.argmax_set(lists[0])) == 6 * M - 3
    _assert_record(got, want[0], lists[0], 1e-6, what="(b)")
    assert tuple(got[f] for f in NAME_FIELDS) == (DR.BOUND, -1, 0, 3, 1) and got["violation"] == 0.25


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["one_nan", "two_inf_across_a_join"])
def test_diagnose_non_finite_control_point(api, torch_cuda, bad):
    """Non-finite control points in the middle instance of three: one NaN; or +inf at the two control points a C0 join ties, c5 of segment 2
    and c0 of segment 3, so that this join is inf - inf (one +inf alone enters every row once and cannot give that).  Every row they enter
    counts as violated with value +inf, the least such row is named with violation = +inf, and the neighbours' records are unchanged byte
    for byte."""
    spec = DC.CLASSES[0]
    M, dim = spec[0], spec[1]
    cls, sol = DC.ref_class(spec), DC.solver(spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, 3, 14)
    finite = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=TOL_RANDOM)
    m, i, k = 2, 5, 1
    x[1].reshape(dim, M, 6)[k, m, i] = bad
    if np.isinf(bad):
        x[1].reshape(dim, M, 6)[k, m + 1, 0] = bad  # the C0 join of segment 3 is inf - inf
    got = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=TOL_RANDOM)
    assert got[0:1].tobytes() == finite[0:1].tobytes() and got[2:3].tobytes() == finite[2:3].tobytes()
    want, lists, _ = _restated(cls, sol, hdr, rows.reshape(-1), off, sfc, x, TOL_RANDOM)
    for q in range(3):
        _assert_record(got[q], want[q], lists[q], TOL_RANDOM, what="instance %d" % q)
    d = got[1]
    assert np.isposinf(d["violation"]) and tuple(d[f] for f in NAME_FIELDS) == (DR.BOUND, -1, m, i, k)
    hit = [r for r in lists[1] if DR.effective(r.value) == np.inf]
    assert sorted(set(r.family for r in hit)) == list(range(DR.FAMILIES)) and np.isposinf(d["worst"]).all()
    assert any(np.isnan(r.value) for r in hit if r.family == DR.EQUALITY)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["corridor_face", "vmax", "lsc_b"])
def test_diagnose_non_finite_row_data(api, torch_cuda, where):
    """The NaN enters through the row's data, the trajectory is finite: ONE face of a corridor (a two-sided row is NaN if either side is --
    fmax alone drops it), a velocity limit of the header, the right-hand side of an LSC row.  The rows it enters count as +inf, the least of
    them is named, and the neighbours' records are unchanged byte for byte."""
    spec = DC.CLASSES[0]
    cls, sol = DC.ref_class(spec), DC.solver(spec)
    hdr, rows, off, sfc, x = DC.random_batch(spec, 3, 15)
    finite = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=TOL_RANDOM)
    if where == "corridor_face":
        sfc[1, 2]["bmax"][0] = np.nan
        fam, first = DR.SFC, (DR.SFC, -1, 2, 0, 0)
    elif where == "vmax":
        hdr[1]["vmax"][1] = np.nan
        fam, first = DR.VEL, (DR.VEL, -1, 0, 2, 1)
    else:
        rows[1, 3, 4, 1]["b"] = np.nan
        fam, first = DR.LSC, (DR.LSC, 3, 4, 1, -1)
    got = sol.diagnose_host(hdr, rows.reshape(-1), off, sfc, x, tol=TOL_RANDOM)
    assert got[0:1].tobytes() == finite[0:1].tobytes() and got[2:3].tobytes() == finite[2:3].tobytes()
    want, lists, _ = _restated(cls, sol, hdr, rows.reshape(-1), off, sfc, x, TOL_RANDOM)
    for q in range(3):
        _assert_record(got[q], want[q], lists[q], TOL_RANDOM, what="instance %d" % q)
    d = got[1]
    assert np.isposinf(d["violation"]) and tuple(d[f] for f in NAME_FIELDS) == first and np.isposinf(d["worst"][fam])
    assert [f for f in range(DR.FAMILIES) if np.isinf(d["worst"][f])] == [fam]
    assert d["violated"][fam] >= finite[1]["violated"][fam] and (np.delete(d["violated"], fam) == np.delete(finite[1]["violated"], fam)).all()
