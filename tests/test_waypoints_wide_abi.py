"""CPU tests of the wide waypoint decision's public surface (include/lscqp.h, "lscqp_waypoints_wide_device" and
"lscqp_plan_set_waypoint_decision"): the names and constants are declared, exported and wrapped, and null or bad arguments are reported
before the device is touched.  tests/test_waypoints_wide_gpu.py and tests/test_waypoints_wide_plan_gpu.py have the rest."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lscqp.h")
NEW = ["lscqp_waypoints_wide_device", "lscqp_grid_reserve_wide", "lscqp_plan_set_waypoint_decision"]
CONSTANTS = {"LSCQP_DECISION_ONE_WORKGROUP": 0, "LSCQP_DECISION_WIDE": 1, "LSCQP_DECISION_AUTO": 2}


def test_names_and_constants_are_declared_exported_and_wrapped(api):
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = api.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, txt), name
        assert name in api.EXPORTED_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
        assert name in raw.replace(txt, ""), name  # (spoken of in a comment too: the contract is written out)
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define %s %d\s*$" % (name, value), txt, flags=re.M), name
        assert getattr(api, name[len("LSCQP_"):]) == value, name
    m = re.search(r"^#define LSCQP_DECISION_AUTO_MIN_AGENTS (\d+)\s*$", txt, flags=re.M)
    assert m and int(m.group(1)) == api.DECISION_AUTO_MIN_AGENTS > 0
    for cls, meth in ((api.Grid, "waypoints_wide"), (api.Grid, "reserve_wide"), (api.Plan, "set_waypoint_decision")):
        assert callable(getattr(cls, meth)), meth
    # the wide entry takes the arguments of the one-workgroup entry
    assert L.lscqp_waypoints_wide_device.argtypes == L.lscqp_waypoints_device.argtypes
    one = re.search(r"int lscqp_waypoints_device\s*\((.*?)\);", txt, flags=re.S).group(1)
    wide = re.search(r"int lscqp_waypoints_wide_device\s*\((.*?)\);", txt, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", one) == re.sub(r"\s+", " ", wide)


def test_null_and_bad_arguments_are_reported(api):
    """Every check below returns before a device call: the same answers with and without a GPU.  (What needs a grid or a plan needs a
    device; the GPU files have those refusals.)"""
    L = api.lib()
    one = (C.c_double * 64)()
    p = C.cast(one, C.c_void_p)
    assert L.lscqp_waypoints_wide_device(None, 3.0, 10, 2, 4, p, p, p, p, p, p, p, p, p, None) == api.ERR_INVALID_ARGUMENT
    assert b"bad argument" in L.lscqp_last_error()
    assert L.lscqp_waypoints_wide_device(None, 3.0, 10, 2, 0, None, None, None, None, None, None, None, None, None, None) == api.ERR_INVALID_ARGUMENT
    assert L.lscqp_grid_reserve_wide(None, 4) == api.ERR_INVALID_ARGUMENT
    for which in (api.DECISION_ONE_WORKGROUP, api.DECISION_WIDE, api.DECISION_AUTO, 3, -1):
        assert L.lscqp_plan_set_waypoint_decision(None, which) == api.ERR_INVALID_ARGUMENT
    assert b"null plan" in L.lscqp_last_error()
