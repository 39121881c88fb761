"""CPU tests of patrol missions (include/lscqp.h, "patrol missions"): lscqp_patrol_host -- the function patrol_kernel runs, on the CPU --
against the numpy restatement (tests/patrol_reference.py) on the constructed table (tests/patrol_cases.py) and over a scripted
back-and-forth, the refusals of lscqp_patrol_check and of the entries' argument checks, the ABI of the new struct and constants.  No device."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import patrol_cases as Cs
from tests import patrol_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lscqp.h")
NEW = ("lscqp_patrol_check", "lscqp_patrol_device", "lscqp_patrol_host", "lscqp_field_exchange_device", "lscqp_plan_set_patrol",
       "lscqp_plan_patrol_buffer")
TABLE = Cs.table()


@pytest.fixture(scope="module")
def solver(api):
    sol = api.Solver(api.make_desc(M=5, dim=3))
    yield sol
    sol.close()


def _run(fn, c):
    """`calls` transitions by fn(state, desired, start, threshold, dim, z_2d, legs, swapped) on copies of the case -> (desired, start, legs, swapped)."""
    d, s = c["desired"].copy(), c["start"].copy()
    legs, sw = np.zeros(len(d), np.int32), np.full(len(d), -7, np.int32)
    for _ in range(c["calls"]):
        fn(c["state"], d, s, c["threshold"], c["dim"], c["z_2d"], legs, sw)
    return d, s, legs, sw


@pytest.mark.parametrize("case", TABLE, ids=[c["name"] for c in TABLE])
def test_the_restatement_takes_the_branch_as_the_table_says(case):
    d, s, legs, sw = _run(PR.transition, case)
    assert sw.tolist() == case["expect"].tolist()
    assert legs.tolist() == (case["legs"] if case["legs"] is not None else case["expect"]).tolist()
    if case["calls"] == 1:
        for a, t in enumerate(sw):
            assert (d[a].tolist(), s[a].tolist()) == ((case["start"][a].tolist(), case["desired"][a].tolist()) if t else
                                                      (case["desired"][a].tolist(), case["start"][a].tolist()))
    else:  # there and back: where it began
        assert d.tobytes() == case["desired"].tobytes() and s.tobytes() == case["start"].tobytes()


@pytest.mark.parametrize("case", TABLE, ids=[c["name"] for c in TABLE])
def test_patrol_host_equals_the_restatement_on_the_table(solver, case):
    want, got = _run(PR.transition, case), _run(solver.patrol_host, case)
    for w, g in zip(want, got):
        assert w.tobytes() == g.tobytes(), case["name"]


@pytest.mark.parametrize("n, dim", [(1, 2), (65, 2), (257, 3)])
def test_patrol_host_equals_the_restatement_on_seeded_batches(solver, n, dim):
    c = Cs.batch(n, seed=n, dim=dim)
    want, got = _run(PR.transition, c), _run(solver.patrol_host, c)
    assert n < 8 or 0 < want[3].sum() < n  # (both ways)
    for w, g in zip(want, got):
        assert w.tobytes() == g.tobytes()


def test_forty_calls_of_a_scripted_back_and_forth(solver):
    def by(fn):
        return Cs.scripted_flight(lambda c: fn(c["state"], c["desired"], c["start"], c["threshold"], c["dim"], c["z_2d"], c["legs"], c["swapped"]))

    want, got = by(PR.transition), by(solver.patrol_host)
    assert len(want) == 40
    for r, (w, g) in enumerate(zip(want, got)):
        for x, y in zip(w, g):
            assert x.tobytes() == y.tobytes(), r
    legs = want[-1][2]
    print("legs after 40 calls:", legs.tolist())
    assert (legs >= 2).all() and len(set(legs.tolist())) > 1  # every agent has been there and back; the legs differ in length
    assert any(w[3].any() and not w[3].all() for w in want)   # a call in which some turn and some do not


def test_the_refusals_of_patrol_check(api):
    api.patrol_check(0.1, 10, 10)
    api.patrol_check(0.0, 1, 1)  # 0 is legal and never turns anyone
    for thr in (-1e-300, -0.1, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(api.LscqpError, match="goal_threshold") as e:
            api.patrol_check(thr, 10, 10)
        assert e.value.code == api.ERR_INVALID_ARGUMENT
    with pytest.raises(api.LscqpError, match="n_agents == n_total") as e:  # a sharded plan: the rule of safety_samples
        api.patrol_check(0.1, 5, 10)
    assert e.value.code == api.ERR_INVALID_ARGUMENT
    assert api.lib().lscqp_patrol_check(None, 1, 1) == api.ERR_INVALID_ARGUMENT


def test_the_entries_check_their_arguments_before_anything_else(api, solver):
    """Refused calls touch nothing: the checks come in front of the device."""
    L = api.lib()
    n = 3
    st, d, s = np.zeros((n, 9)), np.ones((n, 3)), np.zeros((n, 3))
    legs, sw = np.zeros(n, np.int32), np.full(n, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = solver._h
    for entry in (L.lscqp_patrol_host, L.lscqp_patrol_device):
        assert entry(None, n, p(st), p(d), p(s), 0.1, 2, 1.0, p(legs), p(sw), None) == api.ERR_INVALID_ARGUMENT
        assert entry(h, -1, p(st), p(d), p(s), 0.1, 2, 1.0, p(legs), p(sw), None) == api.ERR_INVALID_ARGUMENT
        assert entry(h, n, p(st), p(d), p(s), -0.1, 2, 1.0, p(legs), p(sw), None) == api.ERR_INVALID_ARGUMENT
        assert b"goal_threshold" in L.lscqp_last_error()
        assert entry(h, n, p(st), p(d), p(s), float("nan"), 2, 1.0, p(legs), p(sw), None) == api.ERR_INVALID_ARGUMENT
        assert entry(h, n, p(st), p(d), p(s), 0.1, 4, 1.0, p(legs), p(sw), None) == api.ERR_INVALID_ARGUMENT
        assert entry(h, n, p(st), p(d), p(s), 0.1, 2, float("inf"), p(legs), p(sw), None) == api.ERR_INVALID_ARGUMENT
        assert entry(h, n, p(st), p(d), p(d), 0.1, 2, 1.0, p(legs), p(sw), None) == api.ERR_INVALID_ARGUMENT  # one buffer for both
        for k in (2, 3, 4, 8, 9):
            args = [h, n, p(st), p(d), p(s), 0.1, 2, 1.0, p(legs), p(sw), None]
            args[k] = None
            assert entry(*args) == api.ERR_INVALID_ARGUMENT and b"null buffer" in L.lscqp_last_error()
        assert entry(h, 0, None, None, None, 0.1, 2, 1.0, None, None, None) == api.OK  # nobody: nothing to do, on any machine
    ex = L.lscqp_field_exchange_device
    f, o, di, do = (np.zeros(8, np.int32) for _ in range(4))
    assert ex(-1, 4, p(sw), p(f), p(o), p(di), p(do), None) == api.ERR_INVALID_ARGUMENT
    assert ex(2, 0, p(sw), p(f), p(o), p(di), p(do), None) == api.ERR_INVALID_ARGUMENT
    assert ex(2, 65535 * 1024 + 1, p(sw), p(f), p(o), p(di), p(do), None) == api.ERR_UNSUPPORTED
    assert ex(2, 4, None, p(f), p(o), p(di), p(do), None) == api.ERR_INVALID_ARGUMENT
    assert ex(2, 4, p(sw), p(f), p(f), p(di), p(do), None) == api.ERR_INVALID_ARGUMENT
    assert ex(0, 4, None, None, None, None, None, None) == api.OK
    assert (sw == -7).all() and (d == 1).all() and (s == 0).all() and (legs == 0).all()
    assert L.lscqp_plan_set_patrol(None, None) == api.ERR_INVALID_ARGUMENT
    nb = C.c_uint64(5)
    assert L.lscqp_plan_patrol_buffer(None, 0, C.byref(nb)) is None and nb.value == 0


def test_the_abi_of_the_new_struct_constants_and_entries(api):
    src = r"""
#include <stdio.h>
#include "lscqp.h"
int main(void) {
    printf("%zu %zu %d\n", sizeof(lscqp_patrol_desc), sizeof(lscqp_mission_record), LSCQP_PLAN_BUF_COUNT);
    printf("%d %d %d %d %d %d %d %d %d\n", LSCQP_PATROL_DESIRED, LSCQP_PATROL_START, LSCQP_PATROL_LEGS, LSCQP_PATROL_SWAPPED, LSCQP_PATROL_FIELD,
           LSCQP_PATROL_INIT_D, LSCQP_PATROL_FIELD_OTHER, LSCQP_PATROL_INIT_D_OTHER, LSCQP_PATROL_COUNT);
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "abi.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "abi")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)  # (the header is C)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[0].split() == ["8", "160", "19"]  # the record and the plan's buffer list are where they were
    assert [int(v) for v in out[1].split()] == list(range(9))
    assert C.sizeof(api.PatrolDesc) == 8
    assert (api.PATROL_DESIRED, api.PATROL_START, api.PATROL_LEGS, api.PATROL_SWAPPED, api.PATROL_FIELD, api.PATROL_INIT_D, api.PATROL_FIELD_OTHER,
            api.PATROL_INIT_D_OTHER, api.PATROL_COUNT) == tuple(range(9))
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    L = api.lib()
    for name in NEW:
        assert name in api.EXPORTED_SYMBOLS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, text), name
    for owner, meth in ((api.Plan, "set_patrol"), (api.Plan, "patrol"), (api.Solver, "patrol_device"), (api.Solver, "patrol_host"),
                        (api.Solver, "field_exchange_device")):
        assert callable(getattr(owner, meth))
