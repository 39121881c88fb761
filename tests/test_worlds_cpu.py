"""CPU tests of "each mission over its own world" (include/lscqp.h): the argument checks of the new entries that answer before a device is
needed -- a table of calls through api.lib() with plain ctypes, each with its return code and lscqp_last_error() text, in the style of
tests/test_entry_checks_cpu.py --, the fixed text where there is no device, the shape of the fixture tests/golden/forest_worlds.json, and
the argument handling of tools/closed_loop.py's `worlds=` up to the point a device is needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import world_cases as WLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, NO_DEVICE = 0, 1, 2, 3
NO_DEVICE_TEXT = "no HIP device: lscqp has no CPU fallback"
SFC_MODE = "mode must be LSCQP_SFC_INIT, LSCQP_SFC_FROM_HULL or LSCQP_SFC_FROM_POINT"
NULL_WORLD_OF = "null d_world_of: every agent needs the index of its world"

# lscqp_construct_sfc_worlds_device: its parameters in order with arguments that pass every check ("h" a handle with corridors, "p" some
# non-null address, "ws" a non-null address standing for a set: never followed, every row ends before the device is asked for)
GOOD = [("h", "h"), ("ws", "ws"), ("mode", 1), ("n", 1), ("d_world_of", "p"), ("d_points", "p"), ("d_radius", "p"), ("d_sfc", "p"), ("d_status_out", "p"),
        ("d_order", None), ("d_cost_out", None)]
BUFFERS = ["d_points", "d_radius", "d_sfc", "d_status_out"]
ALL_NULL = dict({k: None for k in BUFFERS}, d_world_of=None)
# (what is wrong, {parameter: value}, return code, text or None) -- the order of the entry it extends: handle, mode, size, the empty batch,
# buffers, then its own argument
TABLE = [
    ("null handle", {"h": None}, INVALID, "null handle"),
    ("null worlds", {"ws": None}, INVALID, "null handle"),
    ("null handle and null buffers", dict(ALL_NULL, h=None), INVALID, "null handle"),
    ("null worlds and a bad mode", {"ws": None, "mode": 3}, INVALID, "null handle"),
    ("mode -1", {"mode": -1}, INVALID, SFC_MODE),
    ("mode 3", {"mode": 3}, INVALID, SFC_MODE),
    ("n < 0", {"n": -1}, INVALID, "negative size"),
    ("bad mode and n < 0", {"mode": 3, "n": -1}, INVALID, SFC_MODE),
    ("bad mode and an empty batch", dict(ALL_NULL, mode=3, n=0), INVALID, SFC_MODE),
    ("n < 0 and null buffers", dict(ALL_NULL, n=-1), INVALID, "negative size"),
    ("n = 0 with null buffers", dict(ALL_NULL, n=0), OK, None),
    ("null d_world_of", {"d_world_of": None}, INVALID, NULL_WORLD_OF),
    ("null d_world_of and a null buffer", {"d_world_of": None, "d_sfc": None}, INVALID, "null buffer"),
] + [("null " + k, {k: None}, INVALID, "null buffer") for k in BUFFERS]


@pytest.fixture(scope="module")
def world(api):
    sol = api.Solver(api.make_desc(M=5, dim=3))
    keep = dict(room=(C.c_double * 512)(), set_room=(C.c_double * 512)())
    yield dict(L=api.lib(), keep=keep, sol=sol, h=sol._h, p=C.cast(keep["room"], C.c_void_p), ws=C.cast(keep["set_room"], C.c_void_p))
    sol.close()


def _run(world, change):
    args = dict(GOOD)
    args.update(change)
    vals = [world[v] if isinstance(v, str) else v for v in args.values()]
    return world["L"].lscqp_construct_sfc_worlds_device(*vals, None), world["L"].lscqp_last_error().decode()


@pytest.mark.parametrize("what,change,rc,text", TABLE, ids=[r[0].replace(" ", "_") for r in TABLE])
def test_worlds_corridor_entry_check(world, what, change, rc, text):
    got, said = _run(world, change)
    assert got == rc, (what, got, said)
    if text is not None:
        assert said == text, what


def test_set_checks_that_need_no_device(api, world):
    """lscqp_worlds_create: no worlds, no list, a null member (behind a member that is never followed); the other entries: null handles."""
    L, vp = world["L"], C.c_void_p
    out = vp()
    two = (vp * 2)(world["ws"].value, None)
    for args, text in (((two, 0, C.byref(out)), "lscqp_worlds_create: at least one world required"),
                       ((two, -3, C.byref(out)), "lscqp_worlds_create: at least one world required"),
                       ((None, 2, C.byref(out)), "lscqp_worlds_create: null argument"),
                       ((two, 2, None), "lscqp_worlds_create: null argument"),
                       ((two, 2, C.byref(out)), "lscqp_worlds_create: map 1 is null")):
        assert L.lscqp_worlds_create(*args) == INVALID and L.lscqp_last_error().decode() == text, text
        assert not out.value
    n = C.c_int32(7)
    assert L.lscqp_worlds_prepare(None, 0.15) == INVALID and L.lscqp_last_error().decode() == "null worlds"
    assert L.lscqp_worlds_info(None, C.byref(n), None, None) == INVALID
    assert L.lscqp_grid_set_worlds(None, None) == INVALID and L.lscqp_last_error().decode() == "null grid"
    assert L.lscqp_grid_download_world(None, 0, None) == INVALID
    assert L.lscqp_plan_set_worlds(None, None) == INVALID and L.lscqp_last_error().decode() == "null plan"
    L.lscqp_worlds_destroy(None)
    with pytest.raises(api.LscqpError) as e:
        api.Worlds([])
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    for name in ("lscqp_worlds_create", "lscqp_worlds_destroy", "lscqp_worlds_prepare", "lscqp_worlds_info", "lscqp_construct_sfc_worlds_device",
                 "lscqp_grid_set_worlds", "lscqp_grid_download_world", "lscqp_plan_set_worlds"):
        assert name in api.EXPORTED_SYMBOLS and hasattr(L, name), name
    # the prototype reader takes the array of handles as a pointer to handles
    assert L.lscqp_worlds_create.argtypes[0] == C.POINTER(C.c_void_p) and L.lscqp_worlds_create.argtypes[2] == C.POINTER(C.c_void_p)


def test_valid_arguments_without_a_device(world):
    """There is no CPU fallback: with every argument in order the entry answers LSCQP_ERR_NO_DEVICE with the one fixed text."""
    n = C.c_int(0)
    if world["L"].hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a device is present; the loud-failure path is for hosts without one")
    assert _run(world, {}) == (NO_DEVICE, NO_DEVICE_TEXT)
    assert _run(world, {"d_order": "p", "d_cost_out": "p"}) == (NO_DEVICE, NO_DEVICE_TEXT)


def test_fixture_shape():
    """Four worlds of 40 pillars in one box, the ten agents of the mission that goes with the first; the helper's missions lie on free nodes
    of their own worlds."""
    g = WLD.fixture()
    assert len(g["worlds"]) == WLD.N_WORLDS == 4 and all(np.array(w).shape == (40, 6) for w in g["worlds"])
    assert g["world_min"] == [-5.0, -5.0, 0.0] and g["world_max"] == [5.0, 5.0, 2.5] and g["resolution"] == 0.1
    assert len(g["starts"]) == len(g["goals"]) == 10 and all(len(p) == 3 for p in g["starts"] + g["goals"])
    B = [np.array(w) for w in g["worlds"]]
    assert all((b[:, 3:] == [0.5, 0.5, 2.5]).all() for b in B)
    assert all(not np.array_equal(B[i], B[j]) for i in range(4) for j in range(i))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "forest_worlds.json")) < 32 * 1024
    off, starts, goals = WLD.seeded_missions([10, 6, 12], seed=1, g=g)
    assert off.tolist() == [0, 10, 16, 28] and starts.shape == goals.shape == (28, 3)
    for k, sl in enumerate(WLD.slices(off)):
        for P in (starts[sl], goals[sl]):
            assert len({tuple(p) for p in P}) == len(P)                      # distinct nodes ...
            assert np.allclose(P[:, :2] * 2, np.round(P[:, :2] * 2))         # ... of the 0.5 m grid
            if k:                                                            # ... clear of world k's pillars
                assert min(np.abs(B[k][:, :2] - p[:2]).max(axis=1).min() for p in P) >= 0.8
    nodes = WLD.seeded_nodes(64, 2, g)
    assert len({tuple(p) for p in nodes}) == 64 and (np.abs(nodes[:, :2]) <= 4.5).all() and (nodes[:, 2] == 1.0).all()


def test_closed_loop_worlds_arguments(tmp_path):
    """tools/closed_loop.py: worlds need missions, exactly one world per mission, and files that exist -- all said before a device is asked for."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import closed_loop

    g = WLD.fixture()
    paths = []
    for k in range(3):
        paths.append(str(tmp_path / ("forest%d.csv" % (k + 1))))
        with open(paths[-1], "w") as f:
            f.write("".join(",".join(repr(v) for v in row) + "\n" for row in g["worlds"][k]))
    (tmp_path / "forest10.csv").write_text("0,0,1,0.5,0.5,2\n")
    world = dict(WLD.world(0, g))
    with pytest.raises(ValueError, match="worlds need missions"):
        closed_loop.run(world, worlds=paths)
    with pytest.raises(ValueError, match="3 worlds for missions=2"):
        closed_loop.run(world, missions=2, worlds=paths)
    with pytest.raises(ValueError, match="no such world file"):
        closed_loop.run(world, missions=3, worlds=paths[:2] + [str(tmp_path / "nowhere.csv")])
    loaded = closed_loop.load_worlds(paths, 3)
    assert [b.shape for b in loaded] == [(40, 6)] * 3 and np.array_equal(loaded[1], np.array(g["worlds"][1]))
    by_dir = closed_loop.load_worlds(str(tmp_path), 4)  # a directory: its CSVs in natural order (forest10 after forest3)
    assert [len(b) for b in by_dir] == [40, 40, 40, 1] and np.array_equal(by_dir[2], loaded[2])
    assert np.array_equal(closed_loop.load_worlds([g["worlds"][0], g["worlds"][3]], 2)[1], np.array(g["worlds"][3]))
