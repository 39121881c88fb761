"""generateCLSC's rows of non-agent obstacles, without a device: the numpy restatement (tests/obstacle_rows_reference.py) against hulls
that state their result by construction and against the agent generator's oracle on the equivalent agent pair; the new entry's place in
the ABI and its argument checks.  The GPU tests (tests/test_obstacle_clsc_gpu.py) hold the kernel to the same packs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import lscgen_cases as LC
from tests import lscgen_checks as T
from tests import obstacle_clsc_cases as OC

CLSC = 1
ENTRY = "lscqp_generate_obstacle_rows_device"


def zero_rows_hold(cases, pk, got):
    """kind "inside": generateCLSC keeps the zero normal, so b = d = (radius + r_own) / 2 exactly; 2-D: n_z == 0 on every segment, the last
    one too (whose record normal has a z component: the obstacle's goal, the origin, is off the plane); tall: on the hull segments"""
    if pk["dim"] == 2:
        assert (got[..., 2] == 0).all()
    elif pk["tall"]:
        assert (got[:, :pk["M"] - 1, :, 2] == 0).all()
    n = 0
    for a in range(pk["N"]):
        for m in range(pk["M"] - 1):
            ci = pk["slot"][a, m]
            if ci >= 0 and cases[ci]["kind"] == "inside":
                assert (got[a, m, :, :3] == 0).all() and (got[a, m, :, 3] == 0.5 * (pk["table"][a]["radius"] + pk["radius"][a])).all(), cases[ci]["name"]
                n += 1
    return n


def hold_rows(cases, pk, got, restated, n_con, n_ref, rows_f32=False, who="device"):
    """The holds of tests/lscgen_checks._hold_device for these packs: constructed result, referee (slivers at their own bar), restatement"""
    tol_b = T.TOL_B_F32 if rows_f32 else T.TOL_B
    sliver, rest = T._family_mask(cases, pk, ("sliver",)), T._family_mask(cases, pk, ("sliver",), keep=False)
    T._hold(got, T._masked(OC.expected_static(cases, pk, n_con), rest), T.TOL_N, tol_b, what="%s clsc obstacle vs constructed" % who)
    T._hold(got, T._masked(OC.expected_static(cases, pk, n_ref), rest), T.TOL_N, tol_b, what="%s clsc obstacle vs referee" % who)
    if sliver.any():
        if rows_f32:
            T._hold(got, T._masked(OC.expected_static(cases, pk, n_ref), sliver), T.ORACLE_DEV["sliver"][0] + 2.0 ** -24, tol_b, what="%s slivers vs referee" % who)
        else:
            T._hold_to_referee(got, T._masked(OC.expected_static(cases, pk, n_ref), sliver), "sliver", what="%s slivers vs referee" % who)
    T._hold(got, restated, T.TOL_N, tol_b, what="%s clsc obstacle vs restatement" % who)


STATIC = [(3, 3, False), (2, 2, False), (2, 3, True)]  # (suite, launch dimension, tall)


@pytest.fixture(scope="module")
def static_packs(oracle):
    out = {}
    for suite, dim, tall in STATIC:
        cases, _, n_ref, n_con = LC.suite(suite)
        pk = OC.pack_static(cases, 6, dim, tall=tall)
        out[(suite, dim, tall)] = (cases, n_ref, n_con, pk, OC.restatement(oracle, pk))
    return out


@pytest.mark.parametrize("key", STATIC, ids=["3d", "2d", "tall"])
def test_restatement_against_constructed_hulls(static_packs, key):
    """One static obstacle per agent, the suites of lscgen_cases on segments 0 .. M-2 at M = 6: the restatement's rows are the constructed
    ones (margin_sum = r_own + radius, obstacle point = the position) at TOL_N / TOL_B; "near" keeps the hull's normal, "inside" gives
    zero rows; the tall type-0 obstacle answers the projected planar case with n_z = 0 whatever the z of the agent's points."""
    cases, n_ref, n_con, pk, rows = static_packs[key]
    T._hold(rows, OC.expected_static(cases, pk, n_con), what="restatement %s vs constructed" % (key,))
    T._hold(rows, OC.expected_static(cases, pk, n_ref), what="restatement %s vs referee" % (key,))
    n_inside = zero_rows_hold(cases, pk, rows)
    assert n_inside > 0 and any(c["kind"] == "near" for c in cases) == (key[0] == 3)
    assert np.isfinite(rows).all() and np.abs(rows[:, pk["M"] - 1, :, :3]).max() > 0


@pytest.mark.parametrize("key", STATIC[:2], ids=["3d", "2d"])
def test_restatement_equals_the_agent_oracle_on_static_obstacles(api, oracle, static_packs, key):
    """Non-tall: the rows are oracle.generate_constraints(CLSC) of the pair whose neighbour flies the predicted points with the obstacle's
    radius and downwash, the planning agent's downwash at 1, goal_all[neighbour] the obstacle goal (here: none, the origin).  Both the hull
    segments and the last one."""
    cases, _, _, pk, rows = static_packs[key]
    want, rec_n = OC.agent_oracle_rows(oracle, pk)
    T._hold(rows, want, what="restatement %s vs agent oracle" % (key,))
    last = pk["M"] - 1
    assert np.array_equal(rows[:, last, :, :3], want[:, last, :, :3])  # (the same segseg_closest and the same float32 steps behind it)
    if pk["dim"] == 2:
        # the plane is z = 0.6 and the obstacle's goal the origin: the RECORD's normal leaves the plane on the last segment, the row does not
        assert (np.abs(rec_n[:, last, 2]) > 1e-3).sum() >= pk["N"] // 4 and (rec_n[:, :last, 2] == 0).all() and (rows[..., 2] == 0).all()


@pytest.mark.parametrize("dim,M", [(3, 5), (3, 2), (2, 5), (2, 2)])
def test_restatement_equals_the_agent_oracle_on_moving_obstacles(api, oracle, dim, M):
    pk = OC.pack_moving(M, dim, n=24, with_tall=False)
    assert (np.abs(pk["table"]["velocity"][:, :2]).max(1) > 0).all()
    rows = OC.restatement(oracle, pk)
    want = OC.agent_oracle_rows(oracle, pk)[0]
    T._hold(rows, want, what="restatement moving %d-D M=%d vs agent oracle" % (dim, M))
    # every hull segment has a normal: no pack member sits inside its obstacle (on the last segment two segments of a plane may cross)
    assert np.abs(rows[:, :M - 1, :, :3]).max(-1).min() > 0 and (np.abs(rows[:, M - 1, :, :3]).max(-1) > 0).any()


def test_a_2d_row_stops_at_the_y_term_when_the_obstacles_goal_is_off_the_plane(api, oracle):
    """Moving obstacles in the plane z = 0.6 with NO obstacle goal points (the origin, as the plan passes it): on the last segment the LSC
    record's normal has a z component and its obstacle point a z between 0 and 0.6.  The 2-D QP's row is n_x (x - p_x) + n_y (y - p_y) >= d
    (src/traj_optimizer.cpp:414-421): the restatement's rows equal d + n_x p_x + n_y p_y of the agent oracle's unpacked records, carry
    n_z = 0, and a row packed with all three terms would be off by up to decimetres."""
    pk = dict(OC.pack_moving(5, 2, n=24, with_tall=False), obstacle_goal=None)
    rows, rec_n = OC.restatement(oracle, pk, records=True)
    want, orc_n = OC.agent_oracle_rows(oracle, pk)
    T._hold(rows, want, what="restatement 2-D z=0.6 origin goals vs agent oracle's records")
    assert (rows[..., 2] == 0).all() and np.array_equal(rec_n, orc_n)
    assert (np.abs(rec_n[:, 4, 2]) > 1e-2).sum() >= 6
    three_terms = LC.oracle_pairs(oracle, api, CLSC, OC.as_agent_pairs(pk))
    assert np.abs(three_terms[:, 4, :, 3] - rows[:, 4, :, 3]).max() > 1e-2


def test_the_tall_rule_flattens_the_hull_only(oracle):
    """A tall obstacle straight above the agent: the hull's z is dropped, so the normal is planar although the points differ in z only
    by much, and the margin takes the unflattened difference (whose z the planar normal does not see)."""
    pk = OC.pack_moving(3, 3, n=8, with_tall=True)
    rows = OC.restatement(oracle, pk)
    assert pk["tall_mask"].any() and (rows[pk["tall_mask"], :2, :, 2] == 0).all() and (rows[~pk["tall_mask"], :2, :, 2] != 0).any()


def test_the_entry_is_declared_once_exported_and_typed(api):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lscqp.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert len(re.findall(r"\b%s\s*\(" % ENTRY, code)) == 1
    assert len(re.findall(r"\b%s\b" % ENTRY, header)) >= 2  # declared, and spoken of in the contract text
    assert ENTRY in api.EXPORTED_SYMBOLS and api.EXPORTED_SYMBOLS.count(ENTRY) == 1
    restype, argtypes = api._prototypes()[ENTRY]
    assert restype is C.c_int and len(argtypes) == 17
    assert argtypes[1] is C.c_int32 and argtypes[3] is C.c_int64 and argtypes[4] is C.c_int32 and argtypes[5] is C.c_int64
    assert argtypes[14] is C.c_int32 and argtypes[15] is C.c_int32 and all(argtypes[i] is C.c_void_p for i in (0, 2, 6, 7, 8, 9, 10, 11, 12, 13, 16))
    f = getattr(api.lib(), ENTRY)
    assert f.argtypes == argtypes and hasattr(api.Solver, "generate_obstacle_rows_device")


def test_the_entry_checks_its_arguments_without_a_device(api):
    """null handle, sizes, mode (BVC: UNSUPPORTED with the cause; anything else: INVALID), the empty batch (OK with null buffers), null
    buffers (d_hdr asked for by LSC only, d_obstacle_goal by neither), then the device."""
    import torch

    L = api.lib()
    sol = api.Solver(api.make_desc(M=5, dim=3))
    buf = (C.c_double * 512)()
    p = C.cast(buf, C.c_void_p)
    par = api.ObstacleParam(1.0, 0.75, 3.0, 0.1, 1, 1)
    pp = C.cast(C.byref(par), C.c_void_p)
    last = lambda: L.lscqp_last_error().decode()  # noqa: E731
    f = getattr(L, ENTRY)
    good = dict(h=sol._h, mode=CLSC, param=pp, n_agents=1, n_dyn=2, first_agent=0, traj=p, ids=p, table=p, ogoal=None, radius=p, goal=p, hdr=None,
                rows=p, n_obs_total=5, slot0=3)

    def call(**kw):
        a = dict(good, **kw)
        return f(*[a[k] for k in good], None)

    assert call(h=None) == api.ERR_INVALID_ARGUMENT and last() == "null handle"
    assert call(param=None) == api.ERR_INVALID_ARGUMENT and last() == "null handle"
    for kw in (dict(n_agents=-1), dict(n_dyn=-1), dict(first_agent=-1), dict(slot0=-1), dict(slot0=4), dict(n_obs_total=1)):
        assert call(**kw) == api.ERR_INVALID_ARGUMENT and last() == "inconsistent sizes (n_obs_total >= slot0 + n_dyn required)", kw
    assert call(h=None, n_agents=-1, mode=7) == api.ERR_INVALID_ARGUMENT and last() == "null handle"  # (the earlier check answers)
    assert call(n_agents=-1, mode=7) == api.ERR_INVALID_ARGUMENT and "inconsistent sizes" in last()
    for mode in (-1, 3, 7):
        assert call(mode=mode) == api.ERR_INVALID_ARGUMENT and last() == "mode must be LSCQP_GEN_LSC or LSCQP_GEN_CLSC", mode
    assert call(mode=api.GEN_BVC) == api.ERR_UNSUPPORTED and "LSCQP_GEN_BVC" in last() and "non-agent" in last()
    assert call(mode=api.GEN_BVC, n_agents=0) == api.ERR_UNSUPPORTED  # (the mode is judged before the empty batch)
    for mode in (api.GEN_LSC, CLSC):
        for kw in (dict(n_agents=0), dict(n_dyn=0, slot0=5)):
            assert call(mode=mode, traj=None, ids=None, table=None, radius=None, goal=None, rows=None, **kw) == api.OK, (mode, kw)
    for name in ("traj", "ids", "table", "radius", "goal", "rows"):
        assert call(**{name: None}) == api.ERR_INVALID_ARGUMENT and last() == "null buffer", name
        assert call(mode=api.GEN_LSC, hdr=p, **{name: None}) == api.ERR_INVALID_ARGUMENT and last() == "null buffer", name
    assert call(mode=api.GEN_LSC, hdr=None) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"  # generateLSC reads the velocity guard's header
    if not torch.cuda.is_available():
        for kw in (dict(), dict(ogoal=p), dict(hdr=p), dict(mode=api.GEN_LSC, hdr=p)):
            assert call(**kw) == api.ERR_NO_DEVICE and last() == "no HIP device: lscqp has no CPU fallback", kw
    sol.close()
