"""CPU tests of the chasing and gaussian obstacles' drives (include/lscqp.h, "chasing and gaussian obstacles"): properties of the restatement
(tests/obstacle_drive_reference.py), lscqp_obstacle_drive_host -- the functions obstacle_drive_kernel runs, on the CPU -- against the
restatement bit for bit, the refusals of lscqp_obstacle_drive_check, the ABI of the new structs and entries.  No device."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import obstacle_drive_cases as Cs
from tests import obstacle_drive_reference as D
from tests import obstacle_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lscqp.h")
NEW = ("lscqp_obstacle_drive_check", "lscqp_obstacles_drive_device", "lscqp_obstacle_drive_host", "lscqp_plan_set_obstacle_drives")
f32 = np.float32


def ulp32(x):
    return float(np.spacing(f32(abs(x))))


@pytest.fixture(scope="module")
def solver(api):
    sol = api.Solver(api.make_desc(M=5, dim=3))
    yield sol
    sol.close()


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

def test_at_replan_0_dt_is_0_and_every_driven_entry_is_at_its_start(api):
    sc = Cs.scenario(api)
    table = sc["table0"].copy()
    D.drive_table(sc["models"], sc["drives"], sc["history"], table, Cs.state_at(0), 0, 0.2)
    for i in (Cs.CHASER_A, Cs.CHASER_B):
        assert (table["position"][i] == f32(sc["models"]["start"][i])).all() and (table["velocity"][i] == 0).all()
    assert (table["position"][Cs.GAUSS] == f32(sc["models"]["start"][Cs.GAUSS])).all()
    assert (table["velocity"][Cs.GAUSS] == f32(sc["drives"]["initial_vel"][Cs.GAUSS])).all()  # (a gaussian obstacle starts at its initial velocity)
    for i in (Cs.STRAIGHT, Cs.PATROL, Cs.HELD):
        assert table[i].tobytes() == sc["table0"][i].tobytes()


@pytest.mark.parametrize("twins", [False, True])
def test_a_chasers_speed_never_exceeds_max_vel_beyond_one_rounding(api, twins):
    """The clamp leaves |v| = max_vel to a few double roundings; the table holds v as float32, each component within 2^-24 of it."""
    sc = Cs.scenario(api, twins)
    tables, counts = Cs.reference_flight(sc, 0.2)
    assert counts["speed_clamp_on"] > 0
    for t in tables:
        for i in (Cs.CHASER_A, Cs.CHASER_B):
            assert D.norm3(t["velocity"][i]) <= sc["drives"]["max_vel"][i] * (1 + 2.0 ** -23)


def test_there_is_no_repulsion_at_or_beyond_q_star():
    c = D.Chasing(radius=0.2, max_vel=0.5, max_acc=1.5, gamma_target=1.0, gamma_obs=3.0)
    args = ((0.0, 0.0, 1.0), (0.1, 0.0, 0.0), (1.0, 0.5, 1.0))
    alone = c.update(*args, [], 0.2, 0.0)
    for dist in (0.8, 0.8000001, 5.0):  # Q* = 2 (0.2 + 0.2)
        assert float(f32(dist)) >= 0.8
        assert c.update(*args, [((dist, 0.0, 1.0), 0.2)], 0.2, 0.0) == alone
    inside = c.update(*args, [((0.79, 0.0, 1.0), 0.2)], 0.2, 0.0)
    assert inside != alone and inside[1][0] < alone[1][0]  # pushed away from the obstacle on +x


def test_the_gaussian_position_is_continuous_across_cycle_boundaries(api):
    """n = floor((t + 1e-5) / cycle) steps up at t = k cycle - 1e-5: just below, the partial step is a whole cycle less 2e-9 s; just above, the
    whole cycle is on the checkpointed side and the partial step is -1e-5 + 1e-9 s.  The two positions differ by the float32 roundings of a
    few additions and by (max_vel + max_acc cycle) 2e-9 m."""
    s = Cs.specs()[Cs.GAUSS]
    g = D.Gaussian(s["start"], s["initial_vel"], s["max_vel"], 0.1, s["acc_history"])
    for k in (1, 2, 7, 30, 59):
        tb = k * 0.1 - 1e-5
        lo, hi = g.at(tb - 1e-9), g.at(tb + 1e-9)
        assert int(math.floor((tb - 1e-9 + 1e-5) / 0.1)) == k - 1 and int(math.floor((tb + 1e-9 + 1e-5) / 0.1)) == k
        tol = 4 * ulp32(max(abs(float(c)) for c in lo[0])) + (s["max_vel"] + s["max_acc"] * 0.1) * 2e-9
        assert max(abs(float(a) - float(b)) for a, b in zip(lo[0], hi[0])) <= tol, (k, lo, hi)


def test_over_max_vel_the_gaussian_obstacle_ignores_its_acceleration():
    g = D.Gaussian((1.0, 2.0, 3.0), (0.5, 0.0, 0.0), 0.5, 0.1, [(1.0, 0.0, 0.0)] * 50)
    D.counts.clear()
    p, v, ended = g.at(3.14)
    assert D.counts["gaussian_over"] == 32 and D.counts["gaussian_under"] == 0 and not ended
    assert [float(c) for c in v] == [0.5, 0.0, 0.0]
    assert abs(float(p[0]) - (1.0 + 0.5 * 3.14)) <= 32 * ulp32(3.0) and (float(p[1]), float(p[2])) == (2.0, 3.0)
    # ... and below it, it follows it: x = 1 + 0.1 t + t^2 / 2 at whole cycles
    g = D.Gaussian((1.0, 2.0, 3.0), (0.1, 0.0, 0.0), 50.0, 0.1, [(1.0, 0.0, 0.0)] * 50)
    p, v, _ = g.at(2.0)
    assert abs(float(p[0]) - (1.0 + 0.2 + 2.0)) <= 21 * ulp32(3.2) and abs(float(v[0]) - 2.1) <= 21 * ulp32(2.1)


# ---- the library's functions on the CPU ------------------------------------------------------------------------------------------------

def host_flight(api, solver, sc, time_step, replans=range(Cs.K)):
    table, ckpt, out = sc["table0"].copy(), np.zeros(len(sc["drives"]), api.OBSTACLE_DRIVE_STATE_DTYPE), []
    for r in replans:
        solver.obstacle_drive_host(sc["models"], sc["drives"], sc["history"], Cs.state_at(r), ckpt, time_step, r, table)
        D.advance_table(sc["models"], table, r, time_step)
        out.append(table.copy())
    return out, ckpt


BOTH_WAYS = (("acc_clamp_on", "acc_clamp_off"), ("speed_clamp_on", "speed_clamp_off"), ("repulsion_inside", "repulsion_outside"),
             ("gaussian_over", "gaussian_under"))


@pytest.mark.parametrize("twins, time_step", [(False, 0.2), (False, 0.15), (True, 0.2)], ids=["step_0.2", "step_0.15", "twins"])
def test_the_host_entry_is_the_restatement_bit_for_bit_over_forty_replans(api, solver, twins, time_step):
    sc = Cs.scenario(api, twins)
    want, counts = Cs.reference_flight(sc, time_step)
    print(sorted(counts.items()))
    for a, b in BOTH_WAYS:  # the scenario takes every branch both ways -- counted by the restatement
        assert counts.get(a, 0) > 0 and counts.get(b, 0) > 0, (a, b, counts)
    assert (counts.get("skip", 0) > 0) == twins          # two chasers on one point: the 1e-5 skip
    assert (counts.get("history_ended", 0) > 0) == (time_step == 0.2)  # 60 accelerations: 6 s of a flight of 8 s (of 6 s at 0.15)
    got, ckpt = host_flight(api, solver, sc, time_step)
    for r in range(Cs.K):
        assert got[r].tobytes() == want[r].tobytes(), (r, [i for i in range(6) if got[r][i].tobytes() != want[r][i].tobytes()])
        assert got[r][Cs.HELD].tobytes() == sc["table0"][Cs.HELD].tobytes()  # the plain HELD entry's sentinel
    assert want[-1]["reserved"][Cs.GAUSS] == (D.HISTORY_ENDED if time_step == 0.2 else 0)
    assert (want[-1]["reserved"][[Cs.CHASER_A, Cs.CHASER_B]] == 0).all()
    # the chasers moved, the checkpoint is at the last replan's whole cycles, and only the gaussian obstacle has one
    assert np.abs(want[-1]["position"][Cs.CHASER_A] - want[0]["position"][Cs.CHASER_A]).max() > 0.1
    n_last = int(math.floor((R.clock_time(Cs.K - 1, time_step) + 1e-5) / 0.1))
    assert list(ckpt["i_done"]) == [0, 0, 0, 0, n_last, 0]


def test_the_checkpoint_follows_a_clock_that_jumps_and_restarts_behind_one_written_backwards(api, solver):
    sc = Cs.scenario(api)
    replans = [0, 1, 2, 10, 3, 53, 54]
    want, _ = Cs.reference_flight(sc, 0.2, replans)
    got, ckpt = host_flight(api, solver, sc, 0.2, replans)
    for k in range(len(replans)):
        assert got[k].tobytes() == want[k].tobytes(), replans[k]
    assert ckpt["i_done"][Cs.GAUSS] == 108


def test_indices_outside_their_tables_are_never_followed(api, solver):
    """What lscqp_obstacle_drive_check refuses does not reach memory either: a target beyond n_total flies to goal[3], a slice beyond
    n_history accelerates by zero and says so."""
    sc = Cs.scenario(api)
    bad = sc["drives"].copy()
    bad["target_agent"][Cs.CHASER_A], bad["goal"][Cs.CHASER_A] = 1000, (1.0, 1.0, 1.0)
    bad["history_first"][Cs.GAUSS] = 10 ** 6
    good = bad.copy()
    good["target_agent"][Cs.CHASER_A], good["history_first"][Cs.GAUSS] = -1, 0
    tables = []
    for drives, hist in ((bad, sc["history"]), (good, np.zeros_like(sc["history"]))):
        t, ck = sc["table0"].copy(), np.zeros(6, api.OBSTACLE_DRIVE_STATE_DTYPE)
        for r in range(5):
            solver.obstacle_drive_host(sc["models"], drives, hist, Cs.state_at(r), ck, 0.2, r, t)
        tables.append(t)
    assert tables[0]["reserved"][Cs.GAUSS] == D.HISTORY_ENDED and tables[1]["reserved"][Cs.GAUSS] == 0
    tables[0]["reserved"][Cs.GAUSS] = 0
    assert tables[0].tobytes() == tables[1].tobytes()


def _refused(api, sc, text, n_history=None, n_total=Cs.N_TOTAL, **kw):
    m, d = sc["models"].copy(), sc["drives"].copy()
    for k, (i, v) in kw.items():
        (m if k.startswith("model_") else d)[k.replace("model_", "")][i] = v
    with pytest.raises(api.LscqpError) as e:
        api.obstacle_drive_check(m, d, len(sc["history"]) if n_history is None else n_history, n_total)
    assert e.value.code == api.ERR_INVALID_ARGUMENT and text in str(e.value), str(e.value)


def test_the_check_refuses_each_case_with_its_cause(api):
    sc = Cs.scenario(api)
    api.obstacle_drive_check(sc["models"], sc["drives"], len(sc["history"]), Cs.N_TOTAL)
    A, G = Cs.CHASER_A, Cs.GAUSS
    _refused(api, sc, "model 0: a drive needs an LSCQP_OBSTACLE_HELD model", kind=(Cs.STRAIGHT, api.DRIVE_CHASING))
    _refused(api, sc, "model 1: a drive needs an LSCQP_OBSTACLE_HELD model", kind=(Cs.PATROL, api.DRIVE_GAUSSIAN))
    _refused(api, sc, "model 2: kind must be LSCQP_DRIVE_NONE, _CHASING or _GAUSSIAN", kind=(A, 3))
    _refused(api, sc, "model 4: kind must be", kind=(G, -1))
    for f, v in (("max_vel", np.nan), ("gamma_target", np.inf), ("gamma_obs", -np.inf), ("goal", (0.0, np.nan, 0.0))):
        _refused(api, sc, "model 2: a field is not finite", **{f: (A, v)})
    for f, v in (("initial_vel", (np.inf, 0.0, 0.0)), ("acc_update_cycle", np.nan), ("max_vel", np.inf)):
        _refused(api, sc, "model 4: a field is not finite", **{f: (G, v)})
    _refused(api, sc, "model 2: a field is not finite", model_start=(A, (0.0, 0.0, np.nan)))
    _refused(api, sc, "model 2: max_vel <= 0", max_vel=(A, 0.0))
    _refused(api, sc, "model 4: max_vel <= 0", max_vel=(G, -0.5))
    _refused(api, sc, "model 4: acc_update_cycle <= 0", acc_update_cycle=(G, 0.0))
    _refused(api, sc, "model 4: acc_update_cycle <= 0", acc_update_cycle=(G, -0.1))
    _refused(api, sc, "model 4: the history slice is empty", history_len=(G, 0))
    _refused(api, sc, "model 4: the history slice lies outside [0, n_history)", history_first=(G, -1))
    _refused(api, sc, "model 4: the history slice lies outside [0, n_history)", history_first=(G, 1))
    _refused(api, sc, "model 4: the history slice lies outside [0, n_history)", n_history=59)
    _refused(api, sc, "model 4: the history slice lies outside [0, n_history)", history_len=(G, 2 ** 31 - 1), history_first=(G, 2 ** 31 - 1))
    _refused(api, sc, "model 2: target_agent outside [-1, n_total)", target_agent=(A, Cs.N_TOTAL))
    _refused(api, sc, "model 2: target_agent outside [-1, n_total)", target_agent=(A, -2))
    _refused(api, sc, "model 2: target_agent outside [-1, n_total)", n_total=0)
    _refused(api, sc, "model 3: max_acc <= 0.01", model_max_acc=(Cs.CHASER_B, 0.01))
    # what does not apply to a kind is not asked of it, and an entry without a drive is not looked at
    ok = sc["drives"].copy()
    ok["acc_update_cycle"][A], ok["history_len"][A], ok["target_agent"][G], ok["kind"][Cs.HELD], ok["max_vel"][Cs.HELD] = 0.0, 0, 99, api.DRIVE_NONE, np.nan
    m = sc["models"].copy()
    m["max_acc"][G] = 0.005
    api.obstacle_drive_check(m, ok, len(sc["history"]), Cs.N_TOTAL)


def test_obstacle_drives_reads_the_mission_files_vocabulary(api):
    s = Cs.specs()
    drives, hist = api.obstacle_drives(s, Cs.N_TOTAL)
    assert list(drives["kind"]) == [0, 0, api.DRIVE_CHASING, api.DRIVE_CHASING, api.DRIVE_GAUSSIAN, 0]
    assert list(drives["target_agent"]) == [-1, -1, 0, -1, -1, -1] and (drives["goal"][Cs.CHASER_B] == (1.5, 1.0, 1.0)).all()
    assert drives["acc_update_cycle"][Cs.GAUSS] == 0.1  # (0 in the file: src/mission.cpp:335-337)
    assert (drives["history_first"][Cs.GAUSS], drives["history_len"][Cs.GAUSS]) == (0, 60) and hist.tobytes() == np.float64(s[Cs.GAUSS]["acc_history"]).tobytes()
    assert list(api.obstacle_models(s)["kind"]) == [api.OBSTACLE_STRAIGHT, api.OBSTACLE_PATROL, 0, 0, 0, 0]  # chasing and gaussian stay HELD
    # drawn histories: one slice per gaussian obstacle, ceil(horizon / cycle) long, clamped to max_acc in norm, a function of the seed
    two = [dict(type="gaussian", start=[0, 0, 1], max_vel=1.0, stddev_acc=2.0, max_acc=1.5, acc_update_cycle=0.25),
           dict(type="gaussian", start=[0, 0, 1], max_vel=1.0, stddev_acc=0.1, max_acc=1.5, acc_update_cycle=0.0, initial_vel={"x": 0.1, "y": 0.2, "z": 0.3})]
    d, h = api.obstacle_drives(two, 1, horizon=10.0, seed=3)
    assert list(d["history_first"]) == [0, 40] and list(d["history_len"]) == [40, 100] and h.shape == (140, 3)
    norm = np.sqrt((h ** 2).sum(1))
    assert norm[:40].max() <= 1.5 * (1 + 1e-15) and (np.abs(norm[:40] - 1.5) < 1e-12).sum() > 5 and norm[40:].max() < 1.0
    assert (d["initial_vel"][1] == (0.1, 0.2, 0.3)).all()
    assert api.obstacle_drives(two, 1, horizon=10.0, seed=3)[1].tobytes() == h.tobytes() != api.obstacle_drives(two, 1, horizon=10.0, seed=4)[1].tobytes()
    api.obstacle_drive_check(api.obstacle_models(two), d, len(h), 1)
    with pytest.raises(ValueError, match="target_agent"):
        api.obstacle_drives([dict(s[Cs.CHASER_A], target_agent=3)], 3)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------

def test_structs_constants_and_symbols_match_the_header(api):
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = api.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in api.EXPORTED_SYMBOLS and api.EXPORTED_SYMBOLS.count(name) == 1 and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    DD, SD = api.OBSTACLE_DRIVE_DTYPE, api.OBSTACLE_DRIVE_STATE_DTYPE
    consts = ["LSCQP_DRIVE_NONE", "LSCQP_DRIVE_CHASING", "LSCQP_DRIVE_GAUSSIAN", "LSCQP_OBSTACLE_HISTORY_ENDED", "LSCQP_OBSTACLE_HELD", "LSCQP_PLAN_OBS_COUNT",
              "LSCQP_PLAN_BUF_COUNT"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lscqp.h"\nint main(){printf("%zu %zu %zu %zu", sizeof(lscqp_obstacle_drive), '
           'sizeof(lscqp_obstacle_drive_state), sizeof(lscqp_obstacle_model), sizeof(lscqp_obstacle));\n'
           + "".join('printf(" %%zu", offsetof(lscqp_obstacle_drive, %s));\n' % f for f in DD.names)
           + "".join('printf(" %%zu", offsetof(lscqp_obstacle_drive_state, %s));\n' % f for f in SD.names)
           + "".join('printf(" %%d", (int)%s);\n' % c for c in consts) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert out[:4] == [DD.itemsize, SD.itemsize, 912, api.OBSTACLE_DTYPE.itemsize] and out[:2] == [96, 56]
    assert out[4:4 + len(DD.names)] == [DD.fields[f][1] for f in DD.names]
    assert out[4 + len(DD.names):4 + len(DD.names) + len(SD.names)] == [SD.fields[f][1] for f in SD.names]
    assert out[4 + len(DD.names) + len(SD.names):] == [api.DRIVE_NONE, api.DRIVE_CHASING, api.DRIVE_GAUSSIAN, api.OBSTACLE_HISTORY_ENDED, api.OBSTACLE_HELD, 3, 19]
    assert "96 bytes" in raw and "56 bytes" in raw  # the header documents the sizes it fixes
    for owner, meth in ((api.Plan, "set_obstacle_drives"), (api.Solver, "obstacles_drive_device"), (api.Solver, "obstacle_drive_host")):
        assert callable(getattr(owner, meth))
    assert callable(api.obstacle_drives) and callable(api.obstacle_drive_check)
    # the header no longer says that chasing and gaussian obstacles are not modelled
    assert "whose motion is not modelled here" not in raw


def test_entries_check_their_arguments_without_a_device(api, solver):
    import torch

    L = api.lib()
    buf = (C.c_double * 512)()
    p = C.cast(buf, C.c_void_p)
    last = lambda: L.lscqp_last_error().decode()  # noqa: E731
    h = solver._h
    for entry in (L.lscqp_obstacles_drive_device, L.lscqp_obstacle_drive_host):
        assert entry(None, p, p, 1, p, 1, p, 1, p, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and last() == "null handle"
        for n_dyn, n_hist, n_total, ts in ((-1, 0, 0, 0.2), (1, -1, 0, 0.2), (1, 0, -1, 0.2), (1, 0, 0, 0.0), (1, 0, 0, -0.2), (1, 0, 0, float("nan")),
                                           (1, 0, 0, float("inf"))):
            assert entry(h, p, p, n_dyn, p, n_hist, p, n_total, p, ts, p, p, None) == api.ERR_INVALID_ARGUMENT and "inconsistent sizes" in last()
        assert entry(h, p, p, solver.max_obstacles() + 1, p, 1, p, 1, p, 0.2, p, p, None) == api.ERR_UNSUPPORTED and "lscqp_max_obstacles" in last()
        assert entry(h, None, None, 0, None, 0, None, 0, None, 0.2, None, None, None) == api.OK  # the empty table: no device either
        for hole in (1, 2, 8, 10, 11):  # models, drives, checkpoints, clock, table
            args = [h, p, p, 1, p, 1, p, 1, p, 0.2, p, p, None]
            args[hole] = None
            assert entry(*args) == api.ERR_INVALID_ARGUMENT and last() == "null buffer", hole
        # a history or a state that is announced must be there; one that is not may be NULL
        assert entry(h, p, p, 1, None, 1, p, 1, p, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"
        assert entry(h, p, p, 1, p, 1, None, 1, p, 0.2, p, p, None) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"
    if not torch.cuda.is_available():
        assert L.lscqp_obstacles_drive_device(h, p, p, 1, p, 1, p, 1, p, 0.2, p, p, None) == api.ERR_NO_DEVICE
        assert last() == "no HIP device: lscqp has no CPU fallback"
    assert L.lscqp_obstacle_drive_host(h, p, p, 1, None, 0, None, 0, p, 0.2, p, p, None) == api.OK  # (zeroed records: no drive)
    assert L.lscqp_plan_set_obstacle_drives(None, p, 1, p, 1) == api.ERR_INVALID_ARGUMENT and last() == "null plan"
    chk = L.lscqp_obstacle_drive_check
    assert chk(None, None, 0, 0, 0) == api.OK
    assert chk(None, p, 1, 0, 0) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"
    assert chk(p, None, 1, 0, 0) == api.ERR_INVALID_ARGUMENT and last() == "null buffer"
    for n, nh, nt in ((-1, 0, 0), (1, -1, 0), (1, 0, -1)):
        assert chk(p, p, n, nh, nt) == api.ERR_INVALID_ARGUMENT and last() == "negative size"
