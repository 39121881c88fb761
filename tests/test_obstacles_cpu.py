"""CPU tests of the dynamic obstacles' host side (include/lscqp.h, "dynamic obstacles in the chain"): the restatement of the reference's
models (tests/obstacle_reference.py) against closed-form facts, lscqp_obstacle_model_prepare against the restatement bit for bit, the
refusals, the ABI of the new structs and entries.  No device.

The two refusals of lscqp_plan_set_obstacles that need a PLAN -- n_dyn > n_obs and constraint_mode != LSCQP_GEN_LSC -- cannot be reached
here (lscqp_plan_create needs a device); tests/test_obstacles_plan_gpu.py holds them.  Here: what the setter answers without a plan."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import obstacle_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lscqp.h")
NEW = ("lscqp_obstacle_model_prepare", "lscqp_obstacles_advance_device", "lscqp_plan_set_obstacles", "lscqp_plan_obstacle_buffer",
       "lscqp_plan_obstacle_upload", "lscqp_plan_obstacle_download")

LONG = dict(start=(-2.0, 0.3, 1.0), goal=(2.5, -0.7, 1.4), radius=0.2, speed=0.8, max_acc=1.6, downwash=1.0)  # dist 4.6 > 2 * 0.2
# (short branch: the reference's t1 = sqrt(dist_to_goal / dist_acc) joins its two parabolas continuously only where dist_acc == max_acc, i.e.
# speed = sqrt(2) max_acc -- chosen so; any other pair jumps at t1 in the reference as well, and the library reproduces the jump)
SHORT = dict(start=(0.1, 0.2, 1.0), goal=(0.4, 0.6, 1.1), radius=0.2, speed=math.sqrt(2.0), max_acc=1.0, downwash=1.0)  # dist 0.51 < 2 * 1


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def test_the_two_straight_branches_are_what_they_are_meant_to_be():
    a, b = R.Straight(**LONG), R.Straight(**SHORT)
    assert a.dist_to_goal > 2 * a.dist_acc and len(a.phases()) == 3
    assert not b.dist_to_goal > 2 * b.dist_acc and len(b.phases()) == 2


@pytest.mark.parametrize("spec", [LONG, SHORT], ids=["long", "short"])
def test_straight_position_is_continuous_at_every_phase_boundary(spec):
    """Just below and at each boundary (t1, t2, t3; t1, t2 in the short branch) the positions agree to float32 rounding of the coordinates."""
    o = R.Straight(**spec)
    check = o.phases()
    for tb in check:
        lo, hi = o.at(np.nextafter(tb, 0.0))[0], o.at(tb)[0]
        tol = 4 * max(ulp32(c) for c in np.concatenate([o.start, o.goal])) + spec["speed"] * 1e-12
        assert np.abs(lo.astype(np.float64) - hi.astype(np.float64)).max() <= tol, (tb, lo, hi)


@pytest.mark.parametrize("spec", [LONG, SHORT], ids=["long", "short"])
def test_straight_rests_at_the_goal_with_zero_velocity_beyond_the_last_phase(spec):
    o = R.Straight(**spec)
    for t in (o.phases()[-1], o.phases()[-1] + 0.2, 1e4):
        p, v = o.at(t)
        assert (p == o.goal).all() and (v == 0).all()
    p, v = o.at(0.0)
    assert (p == o.start).all() and (v == 0).all()


def test_long_branch_flies_at_speed_in_the_middle_and_its_flight_time_is_t3():
    o = R.Straight(**LONG)
    t1, t2, t3 = o.phases()
    assert o.flight_time == pytest.approx(t3, rel=1e-15)
    _, v = o.at(0.5 * (t1 + t2))
    assert math.sqrt(float((v.astype(np.float64) ** 2).sum())) == pytest.approx(LONG["speed"], rel=1e-6)


@pytest.mark.parametrize("nw", [2, 3, 8])
def test_a_patrol_is_back_at_waypoint_0_after_one_lap(nw):
    rng = np.random.default_rng(nw)
    wp = rng.uniform(-2, 2, (nw, 3))
    o = R.Patrol(wp, 0.2, 0.9, 1.8, 1.0)
    lap = o.lap_time()
    assert lap > 0 and all(leg.dist_to_goal > 2 * leg.dist_acc or leg.flight_time > 0 for leg in o.legs)
    p0 = o.at(0.0)[0]
    assert (p0 == wp[0].astype(np.float32)).all()
    # at one lap the repeated subtraction leaves a remainder of rounding size: leg 0 (or the end of the last leg) within ~1e-15 s of
    # waypoint 0, where the obstacle is at rest
    p1, v1 = o.at(lap)
    assert np.abs(p1.astype(np.float64) - p0).max() <= 2 * ulp32(np.abs(wp).max()), (p1, p0)
    assert np.abs(v1).max() <= 1e-6
    # and every leg ends where the next one starts
    for i, leg in enumerate(o.legs):
        assert (leg.goal == o.legs[(i + 1) % nw].start).all()


@pytest.mark.parametrize("start, perpendicular", [((2.0, 0.5, 0.7), True), ((2.0, 0.0, 1.5), False)])
def test_a_spin_keeps_its_radius_and_its_speed(start, perpendicular):
    """Constant spin radius, constant height over the axis point, tangential speed `speed`.  The reference turns the WHOLE offset
    a = start - axis point by 90 degrees for the velocity, its component along the axis included, which that rotation leaves in place:
    with an offset perpendicular to the axis the velocity is the tangential one and its norm is `speed`; otherwise it carries w (a.n)
    along the axis on top -- the reference's own figure, restated as it is."""
    o = R.Spin(axis_point=(0.5, -0.5, 1.0), axis_direction=(0.0, 0.3, 1.0), start=start, radius=0.2, speed=0.7, max_acc=2.0, downwash=1.0)
    n, c = np.array(o.n), np.array(o.axis_point)
    along = float(np.dot(o.a, n))
    assert (abs(along) < 1e-15) == perpendicular
    for t in np.linspace(0, 40, 23):
        p, v = o.at(float(t))
        rel, v = p.astype(np.float64) - c, v.astype(np.float64)
        perp = rel - rel.dot(n) * n
        assert np.linalg.norm(perp) == pytest.approx(o.spin_radius, abs=4 * ulp32(3.0))
        assert rel.dot(n) == pytest.approx(along, abs=4 * ulp32(3.0))  # stays in its plane
        tangential = v - v.dot(n) * n
        assert np.linalg.norm(tangential) == pytest.approx(0.7, abs=4 * ulp32(0.7))
        assert abs(tangential.dot(perp)) <= 1e-5
        assert v.dot(n) == pytest.approx(o.w * along, abs=4 * ulp32(0.7))
        if perpendicular:
            assert np.linalg.norm(v) == pytest.approx(0.7, abs=4 * ulp32(0.7))
    assert (o.at(0.0)[0] == np.array(start, np.float32)).all()


def test_the_clock_counts_whole_nanoseconds():
    assert R.clock_time(0, 0.2) == 0.0 and R.clock_time(5, 0.2) == 1.0 and R.clock_time(3, 0.2) == 0.0 + 1e-9 * 600000000.0
    assert R.clock_time(7, 0.1234567891) == 0.0 + 1e-9 * float(7 * 123456789)
    assert R.clock_time(12345, 0.2) == 2469.0


def _models(api):
    specs = [dict(type="straight", size=0.2, **{k: LONG[k] for k in ("start", "goal", "speed", "max_acc", "downwash")}),
             dict(type="straight", size=0.2, **{k: SHORT[k] for k in ("start", "goal", "speed", "max_acc", "downwash")}),
             dict(type="patrol", size=0.3, speed=0.9, max_acc=1.8, downwash=2.0, waypoints=[[0, 0, 1], {"x": 1.5, "y": 0.25, "z": 1.0}, [0.7, -1.1, 1.3]]),
             dict(type="patrol", size=0.3, speed=0.5, max_acc=0.7, downwash=1.0, waypoints=np.random.default_rng(8).uniform(-3, 3, (8, 3)).tolist()),
             dict(type="spin", size=0.25, speed=0.7, max_acc=2.0, downwash=1.0, start=[2.0, 0.0, 1.5],
                  axis={"pose": {"position": {"x": 0.5, "y": -0.5, "z": 1.0}, "orientation": {"x": 0.0, "y": 0.3, "z": 1.0, "w": 0.0}}}),
             dict(type="chasing", size=0.4, max_acc=1.0, downwash=1.5, start=[1.0, 2.0, 3.0])]
    return api.obstacle_models(specs)


def test_prepare_gives_the_restatements_leg_constants_bit_for_bit(api):
    raw = _models(api)
    m = api.obstacle_model_prepare(raw)
    assert (m["prepared"] == 1).all() and list(m["n_legs"]) == [1, 1, 3, 8, 0, 0]
    for i in range(len(m)):
        o = R.from_model(raw[i])
        legs = [o] if isinstance(o, R.Straight) else (o.legs if isinstance(o, R.Patrol) else [])
        for k, leg in enumerate(legs):
            got = m["leg"][i][k]
            for f in ("start", "goal", "n"):
                assert got[f].tobytes() == getattr(leg, f).astype(np.float32).tobytes(), (i, k, f)
            for f in ("dist_to_goal", "dist_acc", "flight_time"):
                assert np.float64(got[f]).tobytes() == np.float64(getattr(leg, f)).tobytes(), (i, k, f, got[f], getattr(leg, f))
        if isinstance(o, R.Patrol):
            assert np.float64(m["lap_time"][i]).tobytes() == np.float64(o.lap_time()).tobytes()
        if isinstance(o, R.Spin):
            assert m["spin_axis"][i].tobytes() == np.array(o.n).tobytes() and m["spin_offset"][i].tobytes() == np.array(o.a).tobytes()
            assert np.float64(m["spin_w"][i]).tobytes() == np.float64(o.w).tobytes()
    # the caller's fields are left as they were, and legs beyond n_legs are zero
    for f in ("kind", "n_waypoints", "radius", "downwash", "max_acc", "speed", "start", "goal", "waypoints", "axis_point", "axis_direction"):
        assert m[f].tobytes() == raw[f].tobytes(), f
    assert not m["leg"][0][1:].tobytes().strip(b"\0") and not m["leg"][5].tobytes().strip(b"\0")


def _refused(api, m, text, code=None):
    with pytest.raises(api.LscqpError) as e:
        api.obstacle_model_prepare(m)
    assert e.value.code == (api.ERR_INVALID_ARGUMENT if code is None else code) and text in str(e.value), str(e.value)


def test_prepare_refuses_what_the_models_cannot_fly_and_says_why(api):
    good = _models(api)
    api.obstacle_model_prepare(good)
    STRAIGHT, PATROL8, SPIN, HELD = 0, 3, 4, 5

    def bad(i, **kw):
        m = good.copy()
        for k, v in kw.items():
            m[k][i] = v
        return m

    _refused(api, bad(STRAIGHT, speed=0.0), "model 0: speed <= 0")
    _refused(api, bad(PATROL8, speed=-1.0), "model 3: speed <= 0")
    _refused(api, bad(SPIN, max_acc=0.0), "model 4: max_acc <= 0")
    _refused(api, bad(HELD, max_acc=-2.0), "model 5: max_acc <= 0")
    api.obstacle_model_prepare(bad(HELD, speed=0.0))  # (a HELD model has no speed)
    for f, v in (("radius", np.nan), ("downwash", np.inf), ("max_acc", np.nan), ("speed", -np.inf), ("start", (0.0, np.nan, 0.0))):
        _refused(api, bad(STRAIGHT, **{f: v}), "model 0: a field is not finite")
    _refused(api, bad(STRAIGHT, goal=(np.inf, 0, 0)), "model 0: a field is not finite (goal)")
    _refused(api, bad(SPIN, axis_point=(0, 0, np.nan)), "model 4: a field is not finite (axis_point, axis_direction)")
    m = bad(PATROL8)
    m["waypoints"][PATROL8][5][1] = np.nan
    _refused(api, m, "model 3: a field is not finite (waypoints)")
    _refused(api, bad(PATROL8, n_waypoints=9), "model 3: a patrol takes 1 .. LSCQP_OBSTACLE_MAX_WAYPOINTS (8) waypoints")
    _refused(api, bad(PATROL8, n_waypoints=0), "model 3: a patrol takes 1 .. LSCQP_OBSTACLE_MAX_WAYPOINTS (8) waypoints")
    _refused(api, bad(PATROL8, n_waypoints=1), "model 3: the patrol's lap time is not positive")
    m = bad(PATROL8, n_waypoints=3)
    m["waypoints"][PATROL8][:3] = (1.0, 2.0, 3.0)
    _refused(api, m, "model 3: the patrol's lap time is not positive")
    _refused(api, bad(SPIN, axis_direction=(0.0, 0.0, 0.0)), "model 4: the spin's axis direction is zero")
    _refused(api, bad(SPIN, axis_direction=(0.0, 0.0, 2.0), start=(0.5, -0.5, 3.0)), "model 4: the spin's radius is zero")  # on the axis
    _refused(api, bad(STRAIGHT, kind=7), "model 0: kind must be")
    _refused(api, bad(STRAIGHT, radius=-0.1), "model 0: radius < 0")
    # more waypoints than the struct holds, from a mission file
    many = api.obstacle_models([dict(type="patrol", size=0.2, speed=1.0, max_acc=1.0, waypoints=[[i, 0, 1] for i in range(9)])])
    _refused(api, many, "model 0: a patrol takes")


def test_entries_check_their_arguments_without_a_device(api):
    import torch

    L = api.lib()
    sol = api.Solver(api.make_desc(M=5, dim=3))
    buf = (C.c_double * 512)()
    p = C.cast(buf, C.c_void_p)
    last = lambda: L.lscqp_last_error().decode()  # noqa: E731
    adv = L.lscqp_obstacles_advance_device
    assert adv(None, p, 1, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and last() == "null handle"
    for n_dyn, ts in ((-1, 0.2), (1, 0.0), (1, -0.2), (1, float("nan")), (1, float("inf"))):
        assert adv(sol._h, p, n_dyn, ts, p, p, None) == api.ERR_INVALID_ARGUMENT and "inconsistent sizes" in last(), (n_dyn, ts)
    assert adv(sol._h, p, sol.max_obstacles() + 1, 0.2, p, p, None) == api.ERR_UNSUPPORTED and "lscqp_max_obstacles" in last()
    assert adv(sol._h, None, 0, 0.2, None, None, None) == api.OK  # the empty table: nothing asked for, no device either
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert adv(sol._h, args[0], 1, 0.2, args[1], args[2], None) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"
    if not torch.cuda.is_available():
        assert adv(sol._h, p, 1, 0.2, p, p, None) == api.ERR_NO_DEVICE and last() == "no HIP device: lscqp has no CPU fallback"
    par = api.ObstacleParam(1.0, 0.75, 3.0, 0.1, 1, 1)
    m = api.obstacle_model_prepare(_models(api))
    assert L.lscqp_plan_set_obstacles(None, C.byref(par), 1, m.ctypes.data_as(C.c_void_p)) == api.ERR_INVALID_ARGUMENT and last() == "null plan"
    nb = C.c_uint64(7)
    assert L.lscqp_plan_obstacle_buffer(None, 0, C.byref(nb)) is None and nb.value == 0 and last() == "unknown obstacle buffer"
    assert L.lscqp_plan_obstacle_upload(None, 0, p, 0, 8) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_plan_obstacle_download(None, 0, p, 0, 8) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_obstacle_model_prepare(None, 0) == api.OK
    assert L.lscqp_obstacle_model_prepare(None, 1) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"
    assert L.lscqp_obstacle_model_prepare(None, -1) == api.ERR_INVALID_ARGUMENT and last() == "negative size"
    sol.close()


def test_structs_constants_and_symbols_match_the_header(api):
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = api.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in api.EXPORTED_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    fields = ["kind", "n_waypoints", "radius", "start", "goal", "waypoints", "axis_point", "axis_direction", "n_legs", "leg", "lap_time", "spin_axis",
              "spin_offset", "spin_w"]
    leg_fields = ["start", "goal", "n", "dist_to_goal", "flight_time"]
    consts = ["LSCQP_OBSTACLE_MAX_WAYPOINTS", "LSCQP_OBSTACLE_HELD", "LSCQP_OBSTACLE_STRAIGHT", "LSCQP_OBSTACLE_PATROL", "LSCQP_OBSTACLE_SPIN",
              "LSCQP_PLAN_OBS_TABLE", "LSCQP_PLAN_OBS_SAFETY", "LSCQP_PLAN_OBS_CLOCK", "LSCQP_PLAN_OBS_COUNT", "LSCQP_PLAN_BUF_COUNT"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lscqp.h"\nint main(){printf("%zu %zu %zu %zu %zu", sizeof(lscqp_obstacle_model), '
           'sizeof(lscqp_obstacle_leg), sizeof(lscqp_obstacle), sizeof(lscqp_safety_obs), sizeof(lscqp_plan_desc));\n'
           + "".join('printf(" %%zu", offsetof(lscqp_obstacle_model, %s));\n' % f for f in fields)
           + "".join('printf(" %%zu", offsetof(lscqp_obstacle_leg, %s));\n' % f for f in leg_fields)
           + "".join('printf(" %%d", (int)%s);\n' % c for c in consts) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    D, LD = api.OBSTACLE_MODEL_DTYPE, api.OBSTACLE_LEG_DTYPE
    assert out[:5] == [D.itemsize, LD.itemsize, api.OBSTACLE_DTYPE.itemsize, api.SAFETY_OBS_DTYPE.itemsize, C.sizeof(api.PlanDesc)]
    assert out[:2] == [912, 64]
    assert out[5:5 + len(fields)] == [D.fields[f][1] for f in fields]
    assert out[5 + len(fields):5 + len(fields) + len(leg_fields)] == [LD.fields[f][1] for f in leg_fields]
    got = out[5 + len(fields) + len(leg_fields):]
    assert got == [api.OBSTACLE_MAX_WAYPOINTS, api.OBSTACLE_HELD, api.OBSTACLE_STRAIGHT, api.OBSTACLE_PATROL, api.OBSTACLE_SPIN, api.PLAN_OBS_TABLE,
                   api.PLAN_OBS_SAFETY, api.PLAN_OBS_CLOCK, 3, 19]
    for meth in ("set_obstacles", "get_obstacles", "put_obstacles"):
        assert callable(getattr(api.Plan, meth))
    # the header no longer says that obstacles are outside the chain
    assert "are not part of the chain" not in raw and "lscqp_plan_set_obstacles" in raw.replace(txt, "")
