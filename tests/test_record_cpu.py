"""The mission record without a GPU (include/lscqp.h, "the mission record"): the numpy restatement (tests/record_reference.py) against the
reference's own logged mission and summary line, the shim's record -> summary function, and the argument checks that come before the device
is touched."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from tests import helpers as H
from tests import record_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LOG = {}


def _flown_log(threshold):
    """The reference's logged forest10_10 mission -- 160 lines, two per replan of 0.2 s -- as the sample points of 80 replans, every other
    input neutral.  One flight per threshold, shared by the tests."""
    if threshold not in _LOG:
        S = H.load_golden("sim_log_states")
        W = json.load(open(os.path.join(ROOT, "tests", "golden", "forest10_world.json")))
        pos = np.array(S["pos"], np.float64)
        assert pos.shape == (160, 10, 3)
        n = 10
        rec = RR.Record(n, W["goals"], threshold, 0.2)
        ok, one, zero = np.zeros(n, np.int32), np.ones(n, np.int32), np.zeros(n, np.int32)
        for r in range(80):
            rec.step(np.float32(pos[2 * r:2 * r + 2]).transpose(1, 0, 2), pos[2 * r], ok, ok, one, one, zero, 9, RR.neutral_safety(n))
        _LOG[threshold] = (rec.records()[0], pos)
    return _LOG[threshold]


def _polyline(pos):
    return float(sum(RR.vector3_norm(np.float32(pos[1:, a]) - np.float32(pos[:-1, a])).sum() for a in range(pos.shape[1])))


def _summary_fields():
    line = H.load_golden("summary_log_lines")["raw_lines"][1]
    assert "forest10_10.json" in line
    return line.split(",")


def test_the_reference_log_finishes_where_its_summary_says():
    """goal_threshold 0.1 (the launch files'): the first replan that starts within the threshold of every goal is replan 79, so the record has
    replans 80 and flight_time 79 x 0.2 = 15.8 s, the summary's total_flight_time, and its distance -- the float32 polyline through all 160
    logged positions, 103.1626 -- prints as the summary's 103.163."""
    m, pos = _flown_log(0.1)
    f = _summary_fields()
    assert m["finished"] == 1 and m["replans"] == 80
    assert abs(m["flight_time"] - 15.8) <= 1e-12 and float(f[1]) == 15.8
    assert "%g" % m["distance"] == f[2] == "103.163"
    assert abs(m["distance"] - 103.1626) < 5e-5 and abs(m["distance"] - _polyline(pos)) < 1e-9
    assert m["qp_failed"] == m["invalid"] == m["goal_failed"] == m["sfc_kept"] == m["truncated"] == m["waypoint_updates"] == 0
    assert m["first_qp_failed_replan"] == -1 and m["safety_ratio_agent"] == np.inf and m["safety_agent"] == -1


def test_a_wider_threshold_finishes_one_replan_earlier_and_freezes():
    """goal_threshold 0.13: replan 78 already starts within it.  The record is frozen there -- replans 79, flight_time 78 x 0.2, the polyline
    through the first 158 positions (103.0571) -- although the flight went on for another replan."""
    m, pos = _flown_log(0.13)
    assert m["finished"] == 1 and m["replans"] == 79 and abs(m["flight_time"] - 78 * 0.2) <= 1e-12
    assert abs(m["distance"] - 103.0571) < 5e-5 and abs(m["distance"] - _polyline(pos[:158])) < 1e-9


def test_shim_fills_the_summary_line_from_a_record(tmp_path):
    """fillSummaryFromRecord + SimulationSummaryCsv (shim/include/result_csv.hpp) from a small host program: the restatement's record of the
    logged mission, with the safety ratio of the reference's summary, gives the flight-time, distance, safety and excess fields of that
    summary line character for character (and leaves every other field the caller's)."""
    m, _ = _flown_log(0.1)
    f = _summary_fields()
    shim = os.path.join(ROOT, "lsc_dr_planner_amd", "shim")
    exe = tmp_path / "record_summary"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(shim, "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(shim, "test", "record_summary.cpp"), "-o", str(exe)])
    src = tmp_path / "fields.txt"
    other = list(f)
    other[1], other[2], other[3], other[5], other[6] = "-7", "-7", "-7", "-7", "-7"  # (what the record must replace)
    src.write_text("\n".join(other) + "\n")
    args = [repr(float(m["flight_time"])), repr(float(m["distance"])), f[3]] + ["0"] * 6
    out = subprocess.run([str(exe), str(src)] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = out.stdout.strip().split(",")
    assert got[1:4] == f[1:4] == ["15.8", "103.163", "1.02089"] and got[5:7] == f[5:7] == ["0", "0"]
    assert got == f
    # the excess ratios are the float norm() of the three maxima (3, 4, 12 -> 13)
    out = subprocess.run([str(exe), str(src)] + args[:3] + ["3", "4", "12", "0", "0.5", "0"], capture_output=True, text=True, timeout=60)
    assert out.stdout.strip().split(",")[5:7] == ["13", "0.5"]


def test_record_entry_points_validate_their_arguments(api):
    """No GPU needed: these checks come before the device is touched."""
    L = api.lib()
    E = api.ERR_INVALID_ARGUMENT
    h, n64 = C.c_void_p(), C.c_int64(-1)
    d = api.RecordDesc(0.1)
    assert L.lscqp_record_create(None, 10, 1, None, 2, 0.1, 0.2, 1.0, C.byref(d), C.byref(h)) == E
    assert L.lscqp_record_reset(None, None) == E and L.lscqp_record_download(None, None, None) == E
    assert L.lscqp_record_step_device(*([None] * 11)) == E and L.lscqp_record_unfinished(None, None) == E
    assert L.lscqp_record_points(None, None) is None
    L.lscqp_record_destroy(None)
    assert L.lscqp_plan_set_record(None, C.byref(d)) == E and L.lscqp_plan_record(None) is None
    assert L.lscqp_plan_run(None, 10, 1, 1, None, C.byref(n64)) == E and n64.value == 0
    sol = api.Solver(api.make_desc(M=10, dim=2, dt=0.2))
    off = np.array([0, 6, 4, 10], np.int64)
    for args, word in (((0, 1, None, 2, 0.1, 0.2), "n_total"), ((10, 1, None, 0, 0.1, 0.2), "n_samples"), ((10, 1, None, 2, 0.0, 0.2), "record_time_step"),
                       ((10, 1, None, 2, 0.1, 0.0), "time_step"), ((10, 3, off.ctypes.data_as(C.c_void_p), 2, 0.1, 0.2), "mission_offsets")):
        assert L.lscqp_record_create(sol._h, *args, 1.0, C.byref(d), C.byref(h)) == E, word
        assert word in L.lscqp_last_error().decode(), word
    bad = api.RecordDesc(float("nan"))
    assert L.lscqp_record_create(sol._h, 10, 1, None, 2, 0.1, 0.2, 1.0, C.byref(bad), C.byref(h)) == E and "goal_threshold" in L.lscqp_last_error().decode()
    assert L.lscqp_record_create(sol._h, 10, 1, None, 2, 0.1, 0.2, 1.0, None, C.byref(h)) == E
    assert api.MISSION_RECORD_DTYPE.itemsize == 160
    sol.close()
