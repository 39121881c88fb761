"""CPU tests of the grid planner / MAPF layer: lscqp_grid_shape and the ABI of the new entry points, and the test-side restatement
(tests/grid_reference.py) against numbers worked out independently of it and against the one pin the reference's log gives.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

from tests import grid_reference as R
from tests import helpers as H
from tests import waypoint_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_shape_equals_the_restatement(api):
    w = WC.forest10()
    gmin, dims = api.grid_shape(w["world_min"], w["world_max"], 0.5, 2, w["z_2d"])
    assert gmin.tolist() == [-5.0, -5.0, 0.6] and dims.tolist() == [21, 21, 1]
    boxes = [([-5, -5, 0], [5, 5, 2.5], 0.5), ([-5.3, -4.9, 0], [5.2, 5.7, 2.5], 0.5), ([-12, -12, 0], [12, 12, 2.5], 0.5),
             ([0.2, -0.7, 0], [3.1, 0.74, 1], 0.3), ([-1.0, -1.0, 0], [1.0, 1.0, 1], 0.4), ([-7.5, 2.5, 0], [-2.5, 7.5, 2], 0.25)]
    for wmin, wmax, res in boxes:
        for wd in (2, 3):
            gmin, dims = api.grid_shape(wmin, wmax, res, wd, 0.6)
            rmin, rdims = R.grid_shape(wmin, wmax, res, wd, 0.6)
            assert gmin.tolist() == rmin and dims.tolist() == rdims, (wmin, wmax, res, wd)
    # a world box that is not a multiple of the resolution: the grid lies inside it
    gmin, dims = api.grid_shape([-5.3, -4.9, 0], [5.2, 5.7, 2.5], 0.5, 2, 0.6)
    assert gmin.tolist() == [-5.0, -4.5, 0.6] and dims.tolist() == [21, 21, 1]


def test_abi_of_the_waypoint_entry_points(api):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lscqp.h")).read(), flags=re.S)
    for name in ("lscqp_grid_shape", "lscqp_grid_create", "lscqp_grid_destroy", "lscqp_grid_info", "lscqp_grid_download", "lscqp_grid_fields_device",
                 "lscqp_waypoints_device", "lscqp_plan_set_grid"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(api.lib(), name) and name in api.EXPORTED_SYMBOLS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lscqp.h"\nint main(){printf("%zu %zu %zu %d %d %d %d %d\\n", sizeof(lscqp_plan_desc), '
           'offsetof(lscqp_plan_desc, waypoint_mode), offsetof(lscqp_plan_desc, reset_threshold), LSCQP_PLAN_BUF_SAFETY, LSCQP_PLAN_BUF_DESIRED_GOAL, '
           'LSCQP_PLAN_BUF_WAYPOINT_UPDATED, LSCQP_PLAN_BUF_GROUP, LSCQP_PLAN_BUF_COUNT);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    # reserved_ became waypoint_mode in place: the struct's size (96) and every other offset are the ones before
    assert out[:3] == [96, 84, 88]
    assert C.sizeof(api.PlanDesc) == 96 and api.PlanDesc.waypoint_mode.offset == 84 and api.PlanDesc.reset_threshold.offset == 88
    assert out[3:] == [15, 16, 17, 18, 19]
    assert (api.PLAN_SAFETY, api.PLAN_DESIRED_GOAL, api.PLAN_WAYPOINT_UPDATED, api.PLAN_GROUP) == (15, 16, 17, 18)
    assert api.WAYPOINT_FROM_CALLER == 0 and api.WAYPOINT_GRID_PIBT == 1 and api.GRID_UNREACHABLE == R.UNREACHABLE


def _forest10(oracle):
    w = WC.forest10()
    G = WC.reference_grid(oracle, w)
    F, init_d = R.mission_fields(G, w["starts"], w["goals"])
    return w, G, F, init_d


def test_restatement_on_forest10_against_worked_numbers(oracle):
    """Numbers from an independent script (occupancy from the voxel field, BFS, one PIBT step per rollout step)."""
    w, G, F, init_d = _forest10(oracle)
    assert G.gmin == [-5.0, -5.0, 0.6] and G.dims == [21, 21, 1]
    assert int(G.occ.sum()) == 96 and G.occ.size == 441
    for p in w["starts"] + w["goals"]:
        i, j = G.node(p)
        assert not G.occ[j, i]
    assert init_d.tolist() == [26, 22, 20, 22, 26, 26, 22, 20, 22, 26]
    # a grid-only rollout: every agent jumps to its PIBT node (one group, filter off)
    way = np.array(w["starts"], float)
    n = len(way)
    goal_nodes = [G.node(g) for g in w["goals"]]
    steps = None
    for t in range(60):
        _, desired, _, new = R.waypoint_step(G, -1, way, None, way, way, F, init_d, use_filter=False)
        old, nodes = [G.node(p) for p in way], [G.node(p) for p in new]
        assert len(set(nodes)) == n, "vertex conflict at step %d" % t
        for i in range(n):
            for j in range(n):
                assert not (i != j and nodes[i] == old[j] and nodes[j] == old[i]), "swap conflict at step %d" % t
            assert abs(nodes[i][0] - old[i][0]) + abs(nodes[i][1] - old[i][1]) <= 1 and not G.occ[nodes[i][1], nodes[i][0]]
        if t == 0:
            assert new[0][:2].tolist() == [3.5, 0.0]  # the first waypoint the reference's log shows for agent 0
        way = new
        if nodes == goal_nodes:
            steps = t + 1
            break
    assert steps == 26 == int(init_d.max())


def test_logged_waypoints_lie_on_free_nodes(oracle):
    """The one reference-held pin: the 790 waypoints inferred from the reference's log all lie on grid nodes, and at most 8 of them on a
    node the restated occupancy rule calls occupied (a cap: the waypoints were inferred from trajectories, a few are wrong; a wrong rule --
    cell centres instead of cells, a radius off by the voxel size -- misses by dozens).  The rule gives 6."""
    w, G, _, _ = _forest10(oracle)
    replay = H.load_golden("kat_log_pipeline")["replay"]
    assert len(replay) == 790
    bad = []
    for r in replay:
        p = np.array(list(r["waypoint"]) + [w["z_2d"]])
        nd = G.node(p)
        assert np.abs(G.point(nd)[:2].astype(float) - p[:2]).max() <= 1e-4, r
        if G.occ[nd[1], nd[0]]:
            bad.append((r["agent"], r["replan"]))
    print("logged waypoints on occupied nodes:", sorted(bad))
    assert len(bad) <= 8, bad


def test_toy_cases_have_the_worked_answers(oracle):
    for name in WC.TOYS:
        c = WC.toy_case(name)
        G = WC.reference_grid(oracle, c["world"])
        assert (G.occ == c["world"]["occ"]).all(), name  # the pillars make exactly the picture
        F, init_d = R.mission_fields(G, c["starts"], c["goals"])
        if c["init_d"] is not None:
            init_d = np.array(c["init_d"])
        label, desired, updated, new = R.waypoint_step(G, c["range"], c["positions"], None, c["current_goals"], c["waypoints"], F, init_d)
        assert desired.tolist() == c["expect"], (name, desired.tolist(), c["expect"])
        for i in range(len(desired)):
            moved = int(desired[i]) != G.node(c["waypoints"][i])[1] * G.W + G.node(c["waypoints"][i])[0]
            if name == "two_groups":
                continue
            assert updated[i] == int(moved), (name, i)  # one group, no range: whoever PIBT moves takes its waypoint
    # two groups: both head for the same node, and the one whose position is far from it fails the range test of the filter
    c = WC.toy_case("two_groups")
    G = WC.reference_grid(oracle, c["world"])
    F, init_d = R.mission_fields(G, c["starts"], c["goals"])
    label, desired, updated, new = R.waypoint_step(G, c["range"], c["positions"], None, c["current_goals"], c["waypoints"], F, init_d)
    assert label.tolist() == [0, 1] and updated.tolist() == [1, 0]
    assert new[0][:2].tolist() == [1.0, 0.5] and new[1].tolist() == c["waypoints"][1].tolist()


def test_groups_filter_and_unreachable_nodes():
    """The restatement's pieces on hand-made input: connected components through a chain, the sentinel, the find-valid-update loop."""
    occ = np.zeros((3, 7), bool)
    occ[:, 3] = True  # a wall splits the grid
    G = R.Grid([0, 0, 0], [3.0, 1.0, 1.0], 0.5, 0.5, 0.15, occ=occ)
    D = G.field((0, 0))
    assert D[0, 0] == 0 and D[2, 2] == 4 and (D[:, 3:] == R.UNREACHABLE).all()
    pos = [[0, 0, 0], [2.5, 0, 0], [5.0, 0, 0], [20, 0, 0]]
    assert R.groups_of(pos, 3.0) == [[0, 1, 2], [3]]  # 0 and 2 are out of range of each other and joined through 1
    assert R.groups_of(pos, -1) == [[0, 1, 2, 3]]
    assert R.groups_of(pos, 2.0) == [[0], [1], [2], [3]]
    # a follower may not take the node of a leader that is refused its own move (its current goal has not reached its waypoint)
    G = R.Grid([0, 0, 0], [2.0, 0.0, 1.0], 0.5, 0.5, 0.15, occ=np.zeros((1, 5), bool))
    way = np.array([[0.5, 0, 0.5], [1.0, 0, 0.5]])
    goals = np.array([[2.0, 0, 0.5], [2.0, 0, 0.5]])
    F, init_d = R.mission_fields(G, way, goals)
    cg = way.copy()
    _, desired, updated, _ = R.waypoint_step(G, -1, way, None, cg, way, F, init_d)
    assert desired.tolist() == [2, 3] and updated.tolist() == [1, 1]
    cg[1, 0] += 0.3
    _, desired, updated, _ = R.waypoint_step(G, -1, way, None, cg, way, F, init_d)
    assert desired.tolist() == [2, 3] and updated.tolist() == [0, 0]
