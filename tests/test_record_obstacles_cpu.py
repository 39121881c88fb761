"""The obstacle record without a device (include/lscqp.h, "the obstacle record"): the restatement on a hand table whose expected output is
written out by construction, the struct sizes against the header, the entries' argument checks, and the shim's three-argument
fillSummaryFromRecord from a small host program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tests import helpers as H
from tests import record_obstacles_cases as RC
from tests import record_obstacles_reference as ROR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_restatement_on_the_hand_table():
    """tests/record_obstacles_cases.py: hand_table says what each replan shows -- a tie between two agents of one replan (the smaller id), a
    tie across replans (the earlier one), an agent at +inf throughout, a NaN (never taken, not compared), 1.0 (not below one) and the
    double just below it (counted), and a mission that freezes at replan 1 while the others fly on."""
    offsets, steps, missions, agents = RC.hand_table()
    got_m, got_a = ROR.flight(offsets, steps)
    assert got_m == missions
    assert got_a == agents
    assert RC.BELOW < 1.0 and np.nextafter(RC.BELOW, 2.0) == 1.0
    # the same through the struct arrays the device tests compare
    from lsc_dr_planner_amd import api

    ms, ag = ROR.as_arrays(np, api.MISSION_OBSTACLE_RECORD_DTYPE, api.AGENT_OBSTACLE_RECORD_DTYPE, got_m, got_a)
    assert ms["agent"].tolist() == [2, 4, 6] and ms["replan"].tolist() == [2, 1, 2] and ms["compared"].tolist() == [11, 2, 2]
    assert ms["below_one"].tolist() == [3, 2, 0] and ms["safety_ratio_obs"].tolist() == [RC.BELOW, 0.8, 1.0]
    assert np.isposinf(ag["safety_ratio_obs"][[3, 5]]).all() and ag["replan"].tolist() == [1, 3, 2, -1, 1, -1, 2]


def test_a_frozen_mission_takes_nothing_and_a_cleared_record_is_infinite():
    offsets = [0, 2]
    missions, agents = ROR.cleared(offsets)
    assert missions == [dict(safety_ratio_obs=RC.INF, replan=-1, agent=-1, obstacle=-1, sample=-1, below_one=0, compared=0)]
    ROR.accumulate(missions, agents, offsets, [(0.5, 0, 0), (0.25, 1, 1)], finished=[1], replans=[3])
    assert (missions, agents) == ROR.cleared(offsets)
    ROR.accumulate(missions, agents, offsets, [(0.5, 0, 0), (0.25, 1, 1)], finished=[0], replans=[3])
    assert missions[0] == dict(safety_ratio_obs=0.25, replan=3, agent=1, obstacle=1, sample=1, below_one=2, compared=2)


def test_the_dtypes_are_the_headers_structs():
    """40 and 24 bytes as include/lscqp.h says beside the structs, the fields in the header's order, and the spare bytes' constant."""
    from lsc_dr_planner_amd import api

    text = open(os.path.join(ROOT, "include", "lscqp.h")).read()
    for name, dtype in (("lscqp_mission_obstacle_record", api.MISSION_OBSTACLE_RECORD_DTYPE), ("lscqp_agent_obstacle_record", api.AGENT_OBSTACLE_RECORD_DTYPE)):
        m = re.search(r"typedef struct %s \{ /\* (\d+) bytes \*/(.*?)\} %s;" % (name, name), text, flags=re.S)
        assert m, name
        assert dtype.itemsize == int(m.group(1)), name
        body = re.sub(r"/\*.*?\*/", " ", m.group(2), flags=re.S)
        fields = []
        for decl in body.split(";"):
            words = decl.replace(",", " ").split()
            if words:
                kind = {"double": "f8", "int32_t": "i4", "int64_t": "i8"}[words[0]]
                fields += [(w, kind) for w in words[1:]]
        assert [(n, dtype.fields[n][0].str.lstrip("<")) for n in dtype.names] == fields, name
        assert dtype.itemsize == sum(np.dtype(k).itemsize for _, k in fields), name  # (no padding)
    assert api.MISSION_OBSTACLE_RECORD_DTYPE.itemsize == 40 and api.AGENT_OBSTACLE_RECORD_DTYPE.itemsize == 24
    assert int(re.search(r"#define LSCQP_OBSREC_SPARE (\d+)", text).group(1)) == api.OBSREC_SPARE
    for sym in ("lscqp_record_set_obstacle_figures", "lscqp_record_obstacles_download", "lscqp_record_obstacles_raw", "lscqp_plan_set_obstacle_record"):
        assert sym in api.EXPORTED_SYMBOLS and sym in api._prototypes()


def test_the_entries_refuse_null_arguments(api):
    """No GPU needed: these checks come before the device is touched."""
    L = api.lib()
    E = api.ERR_INVALID_ARGUMENT
    assert L.lscqp_record_set_obstacle_figures(None, None) == E and "null record" in L.lscqp_last_error().decode()
    assert L.lscqp_record_obstacles_download(None, None, None) == E
    nb = C.c_uint64(7)
    assert L.lscqp_record_obstacles_raw(None, C.byref(nb)) is None and nb.value == 0
    assert L.lscqp_plan_set_obstacle_record(None, 1) == E and "null plan" in L.lscqp_last_error().decode()


def test_shim_fills_safety_ratio_obs_from_an_obstacle_record(tmp_path):
    """shim/test/record_obstacle_summary.cpp: the two-argument fillSummaryFromRecord leaves safety_ratio_obs the caller's (the file's
    field 4), the three-argument form writes the obstacle record's figure there -- as the stream prints it, +inf as `inf` -- and both fill
    the same other fields."""
    f = H.load_golden("summary_log_lines")["raw_lines"][1].split(",")
    shim = os.path.join(ROOT, "lsc_dr_planner_amd", "shim")
    exe = tmp_path / "record_obstacle_summary"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(shim, "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(shim, "test", "record_obstacle_summary.cpp"), "-o", str(exe)])
    src = tmp_path / "fields.txt"
    other = list(f)
    other[4] = "7.25"  # (the caller's own obstacle figure)
    src.write_text("\n".join(other) + "\n")
    for figure, printed in (("0.987654321", "0.987654"), ("inf", "inf"), ("1", "1")):
        out = subprocess.run([str(exe), str(src), "15.8", "103.1626", f[3], figure], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        two, three = (line.split(",") for line in out.stdout.strip().splitlines())
        assert two[4] == "7.25" and three[4] == printed, (two[4], three[4])
        assert two[:4] == three[:4] == [f[0], "15.8", "103.163", f[3]] and two[5:] == three[5:] == f[5:]
