"""CPU tests of the build's dependency tracking (lsc_dr_planner_amd/build.py): which objects a changed file schedules, read off
build.commands() on the built tree.  Nothing is compiled; every touched file gets its mtime back."""
import os
import time

import pytest

from lsc_dr_planner_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = {"fused_%d_%d_%d_%d_%d%s.o" % (t + (s,)) for t in build.fused_instances() for s in ("", "_sync")}
# every unit that includes csrc/lscqp_internal.hpp (lscsfc_tp.o through lscsfc.hip); lscqp_inst.hip and lscqp_fused.hip do not
INTERNAL = {"api.o", "lscpost.o", "lscrecord.o", "lscgoal.o", "lscsfc.o", "lscsfc_tp.o", "lscqp_comm.o", "lscplan.o", "lscgrid.o", "lscgen.o",
            "lscqp_generic.o", "lscqp_das.o", "lscqp_das_sync.o", "lscqp_prescreen.o", "lscqp_diag.o"}


def scheduled():
    return {os.path.basename(o) for o, _ in build.commands()}


def test_a_built_tree_schedules_nothing():
    assert scheduled() == set(), "the tree is not freshly built (python lsc_dr_planner_amd/build.py)"


@pytest.mark.parametrize("touched, objects", [
    ("lscpost_traj.hpp", {"lscpost.o", "lscrecord.o"}),
    ("lscqp_solve_plan.hpp", {"api.o"}),
    ("lscqp_das_body.inc", {"lscqp_das.o", "lscqp_das_sync.o"} | FUSED),
    ("lscqp_missions.hpp", {"lscgen.o", "lscgrid.o"}),
    ("lscsfc.hip", {"lscsfc.o", "lscsfc_tp.o"}),
    ("lscqp_staging.hpp", {"api.o", "lscsfc.o", "lscsfc_tp.o", "lscqp_comm.o"}),
    ("lscqp_internal.hpp", INTERNAL),
    # (the units that keep host objects; not through lscqp_internal.hpp: the kernels-only units do not need it)
    ("lscqp_device.hpp", {"lscplan.o", "lscgrid.o", "lscrecord.o", "lscsfc.o", "lscsfc_tp.o", "lscqp_diag.o"}),
])
def test_a_touched_file_schedules_exactly_its_dependents(touched, objects):
    path = os.path.join(build.CSRC, touched)
    st = os.stat(path)
    try:
        os.utime(path, (time.time() + 60, time.time() + 60))
        assert scheduled() == objects
    finally:
        os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert scheduled() == set()


def test_commands_are_what_build_runs():
    """commands(force=True): one line per object, the depfile beside it, every unit's flags in their order."""
    cmds = dict(build.commands(force=True))
    assert len(cmds) == len(build.instances()) + 2 * len(build.fused_instances()) + 15
    for o, cmd in cmds.items():
        assert cmd[:1 + len(build.FLAGS)] == [build.HIPCC] + build.FLAGS and cmd[-2:] == ["-o", o]
        assert cmd[cmd.index("-MD"):cmd.index("-c")] == ["-MD", "-MF", o + ".d"]
    flags = {os.path.basename(o): cmd[1 + len(build.FLAGS):cmd.index("-MD")] for o, cmd in cmds.items()}
    assert flags["lscqp_das.o"] == ["-ffp-contract=on"] and flags["lscqp_das_sync.o"] == ["-ffp-contract=on", "-DLSCQP_DAS_FULL_SYNC"]
    assert flags["lscqp_prescreen.o"] == ["-ffp-contract=on"] and flags["lscrecord.o"] == ["-Rpass-analysis=kernel-resource-usage"]
    assert all(flags[f][-1] == "-DLSCQP_DAS_FULL_SYNC" for f in FUSED if f.endswith("_sync.o"))


def test_a_copied_tree_is_judged_by_its_own_files(tmp_path):
    """A depfile names the tree it was written in.  In a built tree that was copied elsewhere, the names under the old csrc/ directory
    (the ../../include ones too) are read under this tree's: nothing is stale, and touching THIS tree's header schedules the object."""
    was = "/some/other/checkout/lsc_dr_planner_amd/csrc"
    o = str(tmp_path / "lscgen.o")
    open(o, "w").close()
    with open(o + ".d", "w") as f:
        f.write("%s: \\\n  %s/lscgen.hip \\\n  %s/lscqp_missions.hpp %s/../../include/lscqp.h\n" % (o, was, was, was))
    seen = []

    def mtime(p, newer=()):
        seen.append(p)
        assert os.path.exists(p), p  # (a named file that is gone would count as newer)
        return float("inf") if os.path.basename(p) in newer else 0.0

    assert not build._stale(o, mtime)
    assert {os.path.join(build.CSRC, "lscgen.hip"), os.path.join(build.CSRC, "lscqp_missions.hpp"),
            os.path.join(build.CSRC, "..", "..", "include", "lscqp.h")} <= set(seen)
    assert build._stale(o, lambda p: mtime(p, newer=("lscqp_missions.hpp",)))
    assert build._stale(o, lambda p: mtime(p, newer=("lscqp.h",)))
